/**
 * @file louvain_kernels.hxx
 * @brief Community detection by multi-level modularity optimisation (grx_louvain), in exact
 * integers: include/essentials_amd.h states the definition.
 *
 * A level graph is a CSR with int32 weights (level 0: the caller's CSR, weight 1 per entry, no
 * weight array: WEIGHTED = false).  A sweep takes the colour classes of grx_color in order, on the
 * schedule of lpa_kernels.hxx: the vertices sorted by (class, row-length bin), one launch per
 * non-empty bin of a wide class, one one-workgroup launch per run of small classes.
 *
 * A decision gathers (label[u], w) per entry other than self entries into a table of (community,
 * weight sum) -- lpa_insert: open addressing, atomicCAS on the key, integer atomicAdd on the
 * sum --, reads tot[key] per occupied slot and reduces twice: to the largest int64 gain
 * k_vc * E - k(v) * t(c), then to the smallest fmix32 among the slots at that gain.  The vertex
 * writes label[v] in place when that gain beats its own label's; the vertices of a class are never
 * adjacent, so they read each other's labels only through tot, and tot changes only when the class
 * is done: louvain_apply_kernel (or the one-workgroup kernel behind its barrier) compares label[v]
 * with the copy taken when the sweep began, which is also what an undone sweep restores.
 *
 *   louvain_init_kernel              label[v] = v, tot[v] = k(v); on level 0 k(v) = the row length.
 *   louvain_group_kernel<G, W>       a class's rows of one bin, G lanes per row (8, or a wavefront).
 *   louvain_block_kernel<BLOCK, W>   a workgroup per row, the table in dynamic LDS; a row with more
 *                                    distinct neighbour communities than half the table goes to ...
 *   louvain_fallback_kernel<W>       ... a table of two slots per entry in global memory.
 *   louvain_apply_kernel             the class's moves: tot[old] -= k(v), tot[new] += k(v), counted.
 *   louvain_narrow_kernel<W>         ONE workgroup: consecutive small classes, decisions and moves.
 *   louvain_inside_kernel<W>, louvain_inside_big_kernel<W>, louvain_squares_kernel
 *                                    the sweep's score: I = the weight inside communities, S = sum tot^2.
 *   louvain_publish_kernel           the sweep's one hand-off: moves, I, S.
 *   louvain_flag_kernel, louvain_renumber_kernel, louvain_compose_kernel, louvain_keys_kernel,
 *   louvain_unpack_kernel, louvain_name_kernel
 *                                    aggregation: communities ranked by their smallest member, the
 *                                    entries keyed (rank[label[u]] << 32) | rank[label[v]] for the
 *                                    sort and the reduction by key, the next CSR from the sorted keys.
 */
#pragma once

#include <gunrock/hip/kernels/lpa_kernels.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

/// Device counters of one call.
struct louvain_counters_t {
  unsigned long long moves;    // labels changed in the sweep that runs
  unsigned long long inside;   // I of the sweep that runs
  unsigned long long squares;  // S of the sweep that runs
  int overflow_n;              // rows on the overflow list of the class that runs
  int pool_at;                 // ... and the units of 4 words their tables take
  int big_n;                   // score: segments on the big list
  int pad;
};
/// What the host reads at a hand-off (words of the pinned mirror).
enum { LOUVAIN_MOVES = 0, LOUVAIN_INSIDE, LOUVAIN_SQUARES, LOUVAIN_WORDS };

/// What every decision reads and writes.
struct louvain_state_t {
  const int32_t* ap;
  const int32_t* aj;
  const int32_t* aw;      // nullptr on level 0: every entry weighs 1
  const int32_t* k;       // k(v): the sum of row v
  int32_t* label;
  const int32_t* before;  // label[] as the sweep began
  int32_t* tot;
  long long entries;      // E of the caller's graph
};

constexpr unsigned long long LOUVAIN_NO_GAIN = 0;  // below every gain in its ordered form

/// An int64 gain as an unsigned word of the same order; never 0, since |gain| < 2^62.
__device__ __forceinline__ unsigned long long louvain_ordered(long long gain) {
  return (unsigned long long)gain ^ 0x8000000000000000ull;
}
/// Smaller for the label that wins among equal gains.
__device__ __forceinline__ unsigned long long louvain_who(int32_t label) {
  return ((unsigned long long)fmix32((unsigned)label) << 32) | (unsigned)label;
}
/// Slot (c, k_vc) of vertex v's table, c not v's own label: keep the better of it and (gain, who).
template <bool NARROW>
__device__ __forceinline__ void louvain_consider(const louvain_state_t& st, int32_t c, int32_t kvc, int32_t kv,
                                                 unsigned long long& gain, unsigned long long& who) {
  const long long t = lpa_load<NARROW>(st.tot + c);
  const unsigned long long g = louvain_ordered((long long)kvc * st.entries - (long long)kv * t);
  const unsigned long long w = louvain_who(c);
  if (g > gain || (g == gain && w < who)) {
    gain = g;
    who = w;
  }
}
/// Does the best other label (ordered gain `best`) beat v's own, of which the row holds own_kvc?
template <bool NARROW>
__device__ __forceinline__ bool louvain_moves(const louvain_state_t& st, int32_t cur, int32_t own_kvc, int32_t kv,
                                              unsigned long long best) {
  if (best == LOUVAIN_NO_GAIN)
    return false;
  const long long t = (long long)lpa_load<NARROW>(st.tot + cur) - kv;
  return best > louvain_ordered((long long)own_kvc * st.entries - (long long)kv * t);
}

template <bool WEIGHTED>
inline __global__ void __launch_bounds__(LPA_BLOCK)
    louvain_init_kernel(const int32_t* ap, int32_t* k, int32_t* label, int32_t* tot, int32_t n) {
  for (int64_t v = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * LPA_BLOCK) {
    if (!WEIGHTED)
      k[v] = ap[v + 1] - ap[v];
    label[v] = (int32_t)v;
    tot[v] = k[v];
  }
}

/**
 * @brief The decision of vertex v (-1: none) by the G lanes of a group, lane l, with the group's
 * table key/sum[0, SLOTS) in LDS; a row has at most SLOTS / 2 entries.  G lanes are part of one
 * wavefront, and every thread of the workgroup calls this the same number of times (two barriers).
 */
template <int G, int SLOTS, bool NARROW, bool WEIGHTED>
__device__ __forceinline__ void louvain_group_decide(const louvain_state_t& st, int32_t v, int32_t* key, int32_t* sum,
                                                     int l) {
  int32_t lo = 0, hi = 0;
  if (v >= 0) {
    lo = st.ap[v];
    hi = st.ap[v + 1];
  }
  for (int s = l; s < SLOTS; s += G) {
    key[s] = LPA_EMPTY;
    sum[s] = 0;
  }
  __syncthreads();
  int fresh = 0;
  for (int32_t e = lo + l; e < hi; e += G) {
    const int32_t u = st.aj[e];
    if (u != v)
      lpa_insert<false>(key, sum, SLOTS, lpa_load<NARROW>(st.label + u), fresh, WEIGHTED ? st.aw[e] : 1);
  }
  __syncthreads();
  if (hi == lo)  // uniform in the group
    return;
  const int32_t cur = lpa_load<NARROW>(st.label + v);
  const int32_t kv = st.k[v];
  unsigned long long mine = LOUVAIN_NO_GAIN, mine_who = ~0ull;
  int32_t own = 0;
  for (int s = l; s < SLOTS; s += G) {
    const int32_t c = key[s];
    if (c == LPA_EMPTY)
      continue;
    if (c == cur)
      own = sum[s];
    else
      louvain_consider<NARROW>(st, c, sum[s], kv, mine, mine_who);
  }
  unsigned long long best = mine;
#pragma unroll
  for (int d = G / 2; d > 0; d >>= 1) {
    const unsigned long long other = __shfl_xor(best, d, G);
    best = other > best ? other : best;
    own = max(own, __shfl_xor(own, d, G));
  }
  unsigned long long who = mine == best ? mine_who : ~0ull;
#pragma unroll
  for (int d = G / 2; d > 0; d >>= 1) {
    const unsigned long long other = __shfl_xor(who, d, G);
    who = other < who ? other : who;
  }
  if (l == 0 && louvain_moves<NARROW>(st, cur, own, kv, best))
    lpa_store<NARROW>(st.label + v, (int32_t)(who & 0xffffffffu));
}

/// The rows rows[0, n_rows) of one class, G lanes each.
template <int G, bool WEIGHTED>
inline __global__ void __launch_bounds__(LPA_BLOCK) louvain_group_kernel(louvain_state_t st, const int32_t* rows, int32_t n_rows) {
  static_assert(G == LPA_SMALL || G == wave_size, "a group is 8 lanes or a wavefront");
  constexpr int SLOTS = G == LPA_SMALL ? LPA_SMALL_SLOTS : LPA_WAVE_SLOTS;
  constexpr int GROUPS = LPA_BLOCK / G;
  __shared__ int32_t s_key[GROUPS * SLOTS], s_sum[GROUPS * SLOTS];
  const int l = threadIdx.x % G;
  const int group = threadIdx.x / G;
  for (int64_t r0 = (int64_t)blockIdx.x * GROUPS; r0 < n_rows; r0 += (int64_t)gridDim.x * GROUPS) {
    const int64_t r = r0 + group;
    louvain_group_decide<G, SLOTS, false, WEIGHTED>(st, r < n_rows ? rows[r] : -1, s_key + group * SLOTS,
                                                    s_sum + group * SLOTS, l);
  }
}

/// LDS words of a workgroup's decision.
struct louvain_block_lds_t {
  unsigned long long best, who;
  int own, fresh, overflow;
};

/**
 * @brief The neighbour communities of row v = entries [lo, hi) summed by the workgroup into
 * key/sum[0, cap).  True when the row has more distinct ones than cap / 2, or an insert found no
 * slot: the table is then of no use.  Every thread calls it; the words of `s` are set for
 * louvain_block_pick.
 */
template <int BLOCK, bool GLOBAL, bool NARROW, bool WEIGHTED>
__device__ __forceinline__ bool louvain_block_count(const louvain_state_t& st, int32_t v, int32_t lo, int32_t hi,
                                                    int32_t* key, int32_t* sum, unsigned cap, louvain_block_lds_t& s) {
  const int tid = threadIdx.x;
  for (unsigned i = tid; i < cap; i += BLOCK) {
    lpa_store<GLOBAL>(key + i, LPA_EMPTY);
    lpa_store<GLOBAL>(sum + i, 0);
  }
  if (tid == 0) {
    s.best = LOUVAIN_NO_GAIN;
    s.who = ~0ull;
    s.own = 0;
    s.fresh = 0;
    s.overflow = 0;
  }
  if (GLOBAL)
    __threadfence();  // the cleared table is at the device's level before any atomic finds it
  __syncthreads();
  constexpr int AHEAD = 4;  // labels gathered before the first insert: their loads overlap
  for (int64_t e0 = (int64_t)lo + tid; e0 < hi; e0 += (int64_t)AHEAD * BLOCK) {
    int32_t c[AHEAD], w[AHEAD];
#pragma unroll
    for (int j = 0; j < AHEAD; ++j) {
      const int64_t e = e0 + (int64_t)j * BLOCK;
      const int32_t u = e < hi ? st.aj[e] : v;  // past the row: skipped like a self entry
      c[j] = u != v ? lpa_load<NARROW>(st.label + u) : LPA_EMPTY;
      w[j] = WEIGHTED && u != v ? st.aw[e] : 1;
    }
    if (__hip_atomic_load(&s.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
      break;
    bool full = false;
#pragma unroll
    for (int j = 0; j < AHEAD; ++j) {
      if (c[j] == LPA_EMPTY || full)
        continue;
      int fresh = 0;
      full = !lpa_insert<GLOBAL>(key, sum, cap, c[j], fresh, w[j]) ||
             (fresh && (unsigned)atomicAdd(&s.fresh, 1) >= cap / 2);
    }
    if (full) {
      __hip_atomic_store(&s.overflow, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      break;
    }
  }
  if (GLOBAL)
    __threadfence();
  __syncthreads();
  return s.overflow != 0;
}

/// The decision of vertex v from the summed table; every thread calls it, after
/// louvain_block_count returned false.  Ends with a barrier: the table and `s` are then free.
template <int BLOCK, bool GLOBAL, bool NARROW>
__device__ __forceinline__ void louvain_block_pick(const louvain_state_t& st, int32_t v, const int32_t* key,
                                                   const int32_t* sum, unsigned cap, louvain_block_lds_t& s) {
  const int tid = threadIdx.x;
  const int32_t cur = lpa_load<NARROW>(st.label + v);
  const int32_t kv = st.k[v];
  unsigned long long mine = LOUVAIN_NO_GAIN, mine_who = ~0ull;
  for (unsigned i = tid; i < cap; i += BLOCK) {
    const int32_t c = lpa_load<GLOBAL>(key + i);
    if (c == LPA_EMPTY)
      continue;
    const int32_t kvc = lpa_load<GLOBAL>(sum + i);
    if (c == cur)
      s.own = kvc;  // one slot holds cur
    else
      louvain_consider<NARROW>(st, c, kvc, kv, mine, mine_who);
  }
  const unsigned long long wave_best = wave_max(mine);
  if (lane_id() == 0 && wave_best != LOUVAIN_NO_GAIN)
    atomicMax(&s.best, wave_best);
  __syncthreads();
  if (mine != LOUVAIN_NO_GAIN && mine == s.best)
    atomicMin(&s.who, mine_who);
  __syncthreads();
  const unsigned long long best = s.best, who = s.who;
  const int32_t own = s.own;
  __syncthreads();  // `s` is read: thread 0 of the next row may set it
  if (tid == 0 && louvain_moves<NARROW>(st, cur, own, kv, best))
    lpa_store<NARROW>(st.label + v, (int32_t)(who & 0xffffffffu));
}

/**
 * @brief A workgroup per row of rows[0, n_rows), the table in dynamic LDS: `max_slots` keys, then
 * as many sums.  A row that overflows goes to over[] as (unit of its table in the pool << 32) | v;
 * the pool gives it 4 words per entry.
 */
template <int BLOCK, bool WEIGHTED>
inline __global__ void __launch_bounds__(BLOCK)
    louvain_block_kernel(louvain_state_t st, const int32_t* rows, int32_t n_rows, int32_t max_slots,
                         unsigned long long* over, louvain_counters_t* ctr) {
  extern __shared__ int32_t s_dyn[];
  __shared__ louvain_block_lds_t s;
  for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const int32_t v = rows[r];
    const int32_t lo = st.ap[v], hi = st.ap[v + 1];
    const unsigned cap = lpa_slots_for(hi - lo, max_slots);
    if (louvain_block_count<BLOCK, false, false, WEIGHTED>(st, v, lo, hi, s_dyn, s_dyn + max_slots, cap, s)) {
      if (threadIdx.x == 0) {
        const int at = atomicAdd(&ctr->pool_at, hi - lo);
        over[atomicAdd(&ctr->overflow_n, 1)] = ((unsigned long long)(unsigned)at << 32) | (unsigned)v;
      }
      __syncthreads();  // `s` is read
      continue;
    }
    louvain_block_pick<BLOCK, false, false>(st, v, s_dyn, s_dyn + max_slots, cap, s);
  }
}

/// The rows on the overflow list, a workgroup each, with a table of two slots per entry in the pool.
template <bool WEIGHTED>
inline __global__ void __launch_bounds__(LPA_BIG_BLOCK)
    louvain_fallback_kernel(louvain_state_t st, const unsigned long long* over, int32_t* pool,
                            const louvain_counters_t* ctr) {
  __shared__ louvain_block_lds_t s;
  const int32_t items = ctr->overflow_n;  // written by the kernel before this one; constant here
  for (int32_t i = blockIdx.x; i < items; i += gridDim.x) {
    const unsigned long long item = over[i];
    const int32_t v = (int32_t)(item & 0xffffffffu);
    const int32_t lo = st.ap[v], hi = st.ap[v + 1];
    const unsigned cap = 2u * (unsigned)(hi - lo);
    int32_t* key = pool + 4 * (std::size_t)(item >> 32);
    // two slots per entry: the table cannot overflow
    louvain_block_count<LPA_BIG_BLOCK, true, false, WEIGHTED>(st, v, lo, hi, key, key + cap, cap, s);
    louvain_block_pick<LPA_BIG_BLOCK, true, false>(st, v, key, key + cap, cap, s);
  }
}

/// The moves of the vertices rows[0, n_rows) of a decided class, applied to tot and counted.
inline __global__ void __launch_bounds__(LPA_BLOCK)
    louvain_apply_kernel(louvain_state_t st, const int32_t* rows, int32_t n_rows, louvain_counters_t* ctr) {
  unsigned long long moved = 0;
  for (int64_t r = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * LPA_BLOCK) {
    const int32_t v = rows[r];
    const int32_t from = st.before[v], to = st.label[v];
    if (from != to) {
      const int32_t kv = st.k[v];
      atomicSub(&st.tot[from], kv);
      atomicAdd(&st.tot[to], kv);
      ++moved;
    }
  }
  moved = wave_sum(moved);
  if (lane_id() == 0 && moved)
    atomicAdd(&ctr->moves, moved);
}

/**
 * @brief ONE workgroup: the classes [c0, c1), each of at most LPA_NARROW_VERTICES vertices, with a
 * barrier between a class's decisions, its moves and the next class.  order[starts[4 c + b] ..
 * starts[4 c + b + 1]) are the rows of bin b of class c.  Dynamic LDS: max(16 wavefront tables,
 * 2 * max_slots) words.  pool: 4 words per entry of the longest row of bins 2 and 3.  Labels and
 * tot pass from class to class inside the launch: agent-scope accesses, fenced before the barrier.
 */
template <bool WEIGHTED>
inline __global__ void __launch_bounds__(LPA_BIG_BLOCK)
    louvain_narrow_kernel(louvain_state_t st, const int32_t* order, const int32_t* starts, int32_t c0, int32_t c1,
                          int32_t max_slots, int32_t* pool, louvain_counters_t* ctr) {
  constexpr int WAVES = LPA_BIG_BLOCK / wave_size;
  extern __shared__ int32_t s_dyn[];
  __shared__ louvain_block_lds_t s;
  const int lane = lane_id();
  const int wave = threadIdx.x / wave_size;
  unsigned long long moved = 0;
  for (int32_t c = c0; c < c1; ++c) {
    const int32_t b0 = starts[LPA_BINS * c], b2 = starts[LPA_BINS * c + 2], b4 = starts[LPA_BINS * c + LPA_BINS];
    for (int32_t r0 = b0; r0 < b2; r0 += WAVES) {
      const int32_t r = r0 + wave;
      louvain_group_decide<wave_size, LPA_WAVE_SLOTS, true, WEIGHTED>(
          st, r < b2 ? order[r] : -1, s_dyn + wave * 2 * LPA_WAVE_SLOTS,
          s_dyn + wave * 2 * LPA_WAVE_SLOTS + LPA_WAVE_SLOTS, lane);
    }
    __syncthreads();  // the tables are the workgroup's now
    for (int32_t r = b2; r < b4; ++r) {
      const int32_t v = order[r];
      const int32_t lo = st.ap[v], hi = st.ap[v + 1];
      unsigned cap = lpa_slots_for(hi - lo, max_slots);
      int32_t *key = s_dyn, *sum = s_dyn + max_slots;
      if (louvain_block_count<LPA_BIG_BLOCK, false, true, WEIGHTED>(st, v, lo, hi, key, sum, cap, s)) {
        __syncthreads();  // `s` is read
        cap = 2u * (unsigned)(hi - lo);
        key = pool;
        sum = pool + cap;
        louvain_block_count<LPA_BIG_BLOCK, true, true, WEIGHTED>(st, v, lo, hi, key, sum, cap, s);
        louvain_block_pick<LPA_BIG_BLOCK, true, true>(st, v, key, sum, cap, s);
      } else {
        louvain_block_pick<LPA_BIG_BLOCK, false, true>(st, v, key, sum, cap, s);
      }
    }
    __threadfence();
    __syncthreads();  // the class is decided: its moves reach tot
    for (int32_t r = b0 + (int32_t)threadIdx.x; r < b4; r += LPA_BIG_BLOCK) {
      const int32_t v = order[r];
      const int32_t from = st.before[v], to = load_relaxed(st.label + v);
      if (from != to) {
        const int32_t kv = st.k[v];
        atomicSub(&st.tot[from], kv);
        atomicAdd(&st.tot[to], kv);
        ++moved;
      }
    }
    __threadfence();
    __syncthreads();  // labels and tot are the next class's input
  }
  moved = wave_sum(moved);
  if (lane == 0 && moved)
    atomicAdd(&ctr->moves, moved);
}

/// inside += the weight of the entries (v, u) with label[v] == label[u]: chunks of LPA_BLOCK rows
/// flattened over the workgroup.  Rows above LPA_INSIDE_SEGMENT entries go to the big list ...
template <bool WEIGHTED>
inline __global__ void __launch_bounds__(LPA_BLOCK)
    louvain_inside_kernel(const int32_t* ap, const int32_t* aj, const int32_t* aw, const int32_t* label, int32_t n,
                          int2* big, louvain_counters_t* ctr) {
  __shared__ int32_t s_pre[LPA_BLOCK], s_base[LPA_BLOCK], s_wave[LPA_BLOCK / wave_size + 1], s_label[LPA_BLOCK];
  const int tid = threadIdx.x;
  unsigned long long inside = 0;
  for (int64_t a = blockIdx.x * (int64_t)LPA_BLOCK; a < n; a += (int64_t)gridDim.x * LPA_BLOCK) {
    const int64_t v = a + tid;
    int32_t lo = 0, d = 0;
    if (v < n) {
      lo = ap[v];
      d = ap[v + 1] - lo;
      s_label[tid] = label[v];
      if (d > LPA_INSIDE_SEGMENT) {
        push_big_segments<LPA_INSIDE_SEGMENT>(&ctr->big_n, big, (int32_t)v, d);
        d = 0;
      }
    }
    flat_walk<LPA_BLOCK>(d, lo, s_pre, s_base, s_wave, [&](int o, int32_t e) {
      if (label[aj[e]] == s_label[o])
        inside += WEIGHTED ? (unsigned long long)aw[e] : 1ull;
    });
    __syncthreads();  // s_label is the next chunk's
  }
  inside = wave_sum(inside);
  if (lane_id() == 0 && inside)
    atomicAdd(&ctr->inside, inside);
}

/// ... which the grid walks a workgroup per segment.
template <bool WEIGHTED>
inline __global__ void __launch_bounds__(LPA_BLOCK)
    louvain_inside_big_kernel(const int32_t* ap, const int32_t* aj, const int32_t* aw, const int32_t* label,
                              const int2* big, louvain_counters_t* ctr) {
  const int32_t items = ctr->big_n;  // written by the kernel before this one; constant here
  unsigned long long inside = 0;
  for (int32_t i = blockIdx.x; i < items; i += gridDim.x) {
    const int2 item = big[i];  // {vertex, segment of its row}
    const int64_t lo = (int64_t)ap[item.x] + (int64_t)item.y * LPA_INSIDE_SEGMENT;
    const int64_t hi = min((int64_t)ap[item.x + 1], lo + LPA_INSIDE_SEGMENT);
    const int32_t mine = label[item.x];
    for (int64_t e = lo + threadIdx.x; e < hi; e += LPA_BLOCK)
      if (label[aj[e]] == mine)
        inside += WEIGHTED ? (unsigned long long)aw[e] : 1ull;
  }
  inside = wave_sum(inside);
  if (lane_id() == 0 && inside)
    atomicAdd(&ctr->inside, inside);
}

/// squares += tot[c]^2 in 64 bits (the sum is at most E^2 < 2^62).
inline __global__ void __launch_bounds__(LPA_BLOCK)
    louvain_squares_kernel(const int32_t* tot, int32_t n, louvain_counters_t* ctr) {
  unsigned long long sum = 0;
  for (int64_t c = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; c < n; c += (int64_t)gridDim.x * LPA_BLOCK) {
    const unsigned long long t = (unsigned long long)tot[c];
    sum += t * t;
  }
  sum = wave_sum(sum);
  if (lane_id() == 0 && sum)
    atomicAdd(&ctr->squares, sum);
}

/// The hand-off that ends a sweep: its moves, I and S, all cleared for the next.
inline __global__ void louvain_publish_kernel(louvain_counters_t* ctr, unsigned long long* mirror, int sequence_slot,
                                       unsigned long long sequence) {
  if (threadIdx.x == 0) {
    mirror[LOUVAIN_MOVES] = ctr->moves;
    mirror[LOUVAIN_INSIDE] = ctr->inside;
    mirror[LOUVAIN_SQUARES] = ctr->squares;
    ctr->moves = 0;
    ctr->inside = 0;
    ctr->squares = 0;
    ctr->big_n = 0;
    stamp_handoff(mirror, sequence_slot, sequence);
  }
}

/// flag[v] = 1 when v is the smallest member of its community (first[]: lpa_first_kernel).
inline __global__ void __launch_bounds__(LPA_BLOCK)
    louvain_flag_kernel(const int32_t* label, const unsigned* first, int32_t n, int32_t* flag) {
  for (int64_t v = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * LPA_BLOCK)
    flag[v] = first[label[v]] == (unsigned)v;
}

/// nid[v] = the rank of v's community among the communities by smallest member (rank[] = the
/// exclusive sum of flag[]); the next level's k(rank) = tot of the community.
inline __global__ void __launch_bounds__(LPA_BLOCK)
    louvain_renumber_kernel(const int32_t* label, const unsigned* first, const int32_t* rank, const int32_t* tot,
                            int32_t n, int32_t* nid, int32_t* next_k) {
  for (int64_t v = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * LPA_BLOCK) {
    const int32_t c = label[v];
    const unsigned head = first[c];
    const int32_t r = rank[head];
    nid[v] = r;
    if (head == (unsigned)v)
      next_k[r] = tot[c];
  }
}

/// comm[o] = nid[comm[o]]: the level vertex of every original vertex.
inline __global__ void __launch_bounds__(LPA_BLOCK) louvain_compose_kernel(int32_t* comm, const int32_t* nid, int32_t n) {
  for (int64_t o = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; o < n; o += (int64_t)gridDim.x * LPA_BLOCK)
    comm[o] = nid[comm[o]];
}

/// comm[o] = first[comm[o]]: the smallest original vertex of the same community.
inline __global__ void __launch_bounds__(LPA_BLOCK) louvain_name_kernel(int32_t* comm, const unsigned* first, int32_t n) {
  for (int64_t o = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; o < n; o += (int64_t)gridDim.x * LPA_BLOCK)
    comm[o] = (int32_t)first[comm[o]];
}

/// Entry e of row v -> key (nid[v] << 32) | nid[aj[e]] and its weight; the row by bisection of ap.
template <bool WEIGHTED>
inline __global__ void __launch_bounds__(LPA_BLOCK)
    louvain_keys_kernel(const int32_t* ap, const int32_t* aj, const int32_t* aw, const int32_t* nid, int32_t n,
                        int64_t entries, unsigned long long* key, int32_t* weight) {
  for (int64_t e = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; e < entries; e += (int64_t)gridDim.x * LPA_BLOCK) {
    int32_t lo = 0, hi = n;  // the last v in [0, n) with ap[v] <= e
    while (hi - lo > 1) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if ((int64_t)ap[mid] <= e)
        lo = mid;
      else
        hi = mid;
    }
    key[e] = ((unsigned long long)(unsigned)nid[lo] << 32) | (unsigned)nid[aj[e]];
    weight[e] = WEIGHTED ? aw[e] : 1;
  }
}

/// The next CSR from the m sorted distinct keys: aj[i] = the key's low word, ap[r] = the first
/// position whose high word is at least r (r = 0 .. n_next).
inline __global__ void __launch_bounds__(LPA_BLOCK)
    louvain_unpack_kernel(const unsigned long long* key, int32_t m, int32_t n_next, int32_t* ap, int32_t* aj) {
  const int64_t stride = (int64_t)gridDim.x * LPA_BLOCK;
  for (int64_t i = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; i < m; i += stride)
    aj[i] = (int32_t)(key[i] & 0xffffffffu);
  for (int64_t r = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; r <= n_next; r += stride) {
    int32_t lo = 0, hi = m;
    while (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if ((key[mid] >> 32) < (unsigned long long)r)
        lo = mid + 1;
      else
        hi = mid;
    }
    ap[r] = lo;
  }
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

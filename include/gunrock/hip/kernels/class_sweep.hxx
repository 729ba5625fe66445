/**
 * @file class_sweep.hxx
 * @brief The colour-class sweep that grx_lpa and grx_louvain share: the schedule, the table and
 * the kernels that decide the vertices of one colour class at once, templated on a decision D.
 *
 * A sweep takes the colour classes of grx_color in order; the vertices of a class are never
 * adjacent.  The vertices are sorted once by (class, row-length bin).  A decision gathers
 * (label[u], weight) per entry of row v other than self entries into a table of (label, sum) --
 * open addressing, atomicCAS on the key, integer atomicAdd on the sum, at most half full, so the
 * table does not depend on the order of the inserts --, scores every occupied slot, reduces to the
 * best score and then to the tie-break among the slots that hold it, and label[v] is written in
 * place when D says the vertex moves.
 *
 *   lpa_starts_kernel            first position of every (class, bin) key in the sorted keys.
 *   lpa_entries_kernel           row entries per (class, bin).
 *   sweep_group_kernel<D, G>     a class's rows of one bin, G lanes per row: 8 lanes and 64 slots for
 *                                short rows, a wavefront and 512 slots up to 256 entries; static LDS.
 *   sweep_block_kernel<D, BLOCK> a workgroup per row, the table in dynamic LDS, two slots per entry
 *                                up to `max_slots`.  A row with more distinct labels than half the
 *                                table overflows and goes to a list ...
 *   sweep_fallback_kernel<D>     ... whose rows get a table of two slots per entry in global memory:
 *                                the same inserts with agent-scope accesses, a workgroup per row.
 *   sweep_narrow_kernel<D>       ONE workgroup runs consecutive small classes with a barrier between
 *                                them: a wavefront per row up to 256 entries, the workgroup per row
 *                                above, the global table in place when the LDS table overflows.
 *   lpa_first_kernel             the smallest vertex id per label.
 *   sweep_inside_kernel<W, C>, sweep_inside_big_kernel<W, C>, sweep_squares_kernel
 *                                the score of a labelling in integers: I = the weight of the entries
 *                                inside communities, S = the sum of tot^2.
 *
 * Within a wide launch labels are read of other classes and written of this one: nothing is handed
 * between workgroups inside a launch.  The one-workgroup kernel does hand a class's results to the
 * next class; there (NARROW) they are read and written with agent-scope relaxed accesses behind the
 * workgroup's barrier.
 *
 * The decision D is a struct of static device functions and types, resolved at compile time
 * (lpa_decision_t in lpa_kernels.hxx, louvain_decision_t<WEIGHTED> in louvain_kernels.hxx):
 *
 *   state_t, counters_t     what a decision reads and writes (ap, aj, label, ...); the call's device
 *                           counters, with `overflow_n` and `pool_at` next to each other.
 *   self_t, self<N>(st, v)  what the scan knows of v itself; self_t::cur is v's label.
 *   tally_t, flush<N>(t, ctr)   what a thread counts over a kernel, and where it goes at the end.
 *   wants<N>(st, v)         does v decide in this sweep?
 *   weight(st, e)           the weight of entry e.
 *   tie_t, no_tie, own_competes, consider<N>(st, self, label, sum, score, tie)
 *                           keep the better of (score, tie) and the slot's; score 0 is "no slot".
 *                           own_competes: the slot of v's own label is considered like any other
 *                           (its sum is handed to decided() either way).
 *   first_tie(a, b), offer(word, tie), label_of(tie)
 *                           the tie-break among lanes (shuffles) and in LDS, and the label it names.
 *   decided<N, WIDTH>(st, v, lo, hi, lane, self, own, best, label, tally)
 *                           the end of a decision, by the WIDTH threads of the row: does the best
 *                           slot (score `best`, naming `label`) beat v's own label, whose slot holds
 *                           `own`?  If so thread 0 writes label[v]; and whatever the decision does
 *                           beside the write-back.
 *   class_done(st, order, b0, b4, tally)   the one-workgroup kernel, when rows order[b0, b4) of a
 *                           class are decided and before the barrier that ends the class.
 *   apply_kernel            host side: the launch that follows a wide class, or nullptr.
 */
#pragma once

#include <gunrock/hip/kernels/row_walk.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int LPA_BLOCK = 256;
constexpr int LPA_BIG_BLOCK = 1024;     // workgroup of a big row, of the fallback and of the narrow kernel
constexpr int LPA_SMALL = 8;            // lanes of a short row
constexpr int LPA_SMALL_SLOTS = 64;     // ... its table
constexpr int LPA_SMALL_ROW = 32;       // ... and its most entries
constexpr int LPA_WAVE_SLOTS = 512;     // table of a wavefront's row
constexpr int LPA_WAVE_ROW = 256;       // ... which has at most this many entries
constexpr int LPA_MIN_SLOTS = 64;       // smallest table of the workgroup path
constexpr int LPA_BIG_ROW = 4096;       // default: longer rows get 1024 threads and the largest table
constexpr int LPA_NARROW_EDGES = 16384; // default: most entries of a class of the narrow kernel
constexpr int LPA_NARROW_VERTICES = 1024;
constexpr int LPA_BINS = 4;             // short, wavefront, medium workgroup, big workgroup
constexpr int LPA_INSIDE_SEGMENT = 4096;  // score: longer rows are cut into segments of this many entries
constexpr int32_t LPA_EMPTY = -1;

/// Bin of a row of `len` entries; b[0..2]: the most entries of a short, a wavefront and a medium row.
__host__ __device__ __forceinline__ unsigned lpa_bin_of(int32_t len, const int32_t* b) {
  return len <= b[0] ? 0u : len <= b[1] ? 1u : len <= b[2] ? 2u : 3u;
}

/// Sort key of vertex v: its colour class, then its bin.
struct lpa_key_t {
  const int32_t* color;
  const int32_t* ap;
  int32_t b[3];
  __host__ __device__ unsigned operator()(int32_t v) const {
    return (unsigned)color[v] * LPA_BINS + lpa_bin_of(ap[v + 1] - ap[v], b);
  }
};

template <bool AGENT, typename T>
__device__ __forceinline__ T lpa_load(const T* p) {
  return AGENT ? load_relaxed(p) : *p;
}
template <bool AGENT, typename T>
__device__ __forceinline__ void lpa_store(T* p, T x) {
  if (AGENT)
    store_relaxed(p, x);
  else
    *p = x;
}

/// Count label l in the table key/cnt[0, cap), `w` times (an entry's weight): `fresh` += 1 when
/// this call took a slot.  False when `cap` probes found neither l nor an empty slot.  GLOBAL: the
/// table is in global memory.
template <bool GLOBAL>
__device__ __forceinline__ bool lpa_insert(int32_t* key, int32_t* cnt, unsigned cap, int32_t l, int& fresh,
                                           int32_t w = 1) {
  unsigned s = __umulhi((unsigned)l * 0x9e3779b1u, cap);
  for (unsigned probe = 0; probe < cap; ++probe) {
    int32_t seen = GLOBAL ? load_relaxed(&key[s]) : __hip_atomic_load(&key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (seen == LPA_EMPTY) {
      seen = atomicCAS(&key[s], LPA_EMPTY, l);
      if (seen == LPA_EMPTY) {
        ++fresh;
        seen = l;
      }
    }
    if (seen == l) {
      atomicAdd(&cnt[s], w);
      return true;
    }
    if (++s == cap)
      s = 0;
  }
  return false;
}

/// Slots of the LDS table of a row of `len` entries: two per entry, within [LPA_MIN_SLOTS, max_slots].
__host__ __device__ __forceinline__ unsigned lpa_slots_for(int32_t len, int32_t max_slots) {
  const long long want = 2ll * len;
  return (unsigned)(want < LPA_MIN_SLOTS ? LPA_MIN_SLOTS : want > max_slots ? max_slots : want);
}

/// starts[k] = first position of key k in the sorted keys (k = 0 .. n_keys).
inline __global__ void __launch_bounds__(LPA_BLOCK)
    lpa_starts_kernel(const unsigned* keys, int32_t n, int32_t n_keys, int32_t* starts) {
  for (int64_t k = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; k <= n_keys; k += (int64_t)gridDim.x * LPA_BLOCK) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if (keys[mid] < (unsigned)k)
        lo = mid + 1;
      else
        hi = mid;
    }
    starts[k] = lo;
  }
}

/// entries[k] += the row lengths of the vertices of key k; a wavefront whose 64 positions share a
/// key adds once.
inline __global__ void __launch_bounds__(LPA_BLOCK)
    lpa_entries_kernel(const unsigned* keys, const int32_t* order, const int32_t* ap, int32_t n,
                       unsigned long long* entries) {
  const int lane = lane_id();
  const int64_t stride = (int64_t)gridDim.x * LPA_BLOCK;
  for (int64_t p0 = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x - lane; p0 < n; p0 += stride) {
    const int64_t p = p0 + lane;
    unsigned k = 0xffffffffu;
    unsigned long long d = 0;
    if (p < n) {
      k = keys[p];
      const int32_t v = order[p];
      d = (unsigned long long)(ap[v + 1] - ap[v]);
    }
    const unsigned k0 = __shfl(k, 0, wave_size);
    if (__all(k == k0)) {  // a whole wavefront inside n: k0 is a key
      d = wave_sum(d);
      if (lane == 0 && d)
        atomicAdd(&entries[k0], d);
    } else if (p < n && d) {
      atomicAdd(&entries[k], d);
    }
  }
}

/**
 * @brief The decision of vertex v (-1: none) by the G lanes of a group, lane l, with the group's
 * table key/sum[0, SLOTS) in LDS; a row has at most SLOTS / 2 entries.  G lanes are part of one
 * wavefront, and every thread of the workgroup calls this the same number of times (two barriers).
 */
template <class D, int G, int SLOTS, bool NARROW>
__device__ __forceinline__ void sweep_group_decide(const typename D::state_t& st, int32_t v, int32_t* key, int32_t* sum,
                                                   int l, typename D::tally_t& tally) {
  int32_t lo = 0, hi = 0;
  if (v >= 0 && D::template wants<NARROW>(st, v)) {
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
      lpa_insert<false>(key, sum, SLOTS, lpa_load<NARROW>(st.label + u), fresh, D::weight(st, e));
  }
  __syncthreads();
  if (hi == lo)  // uniform in the group
    return;
  const typename D::self_t self = D::template self<NARROW>(st, v);
  unsigned long long mine = 0;
  typename D::tie_t mine_tie = D::no_tie;
  int32_t own = 0;
  for (int s = l; s < SLOTS; s += G) {
    const int32_t k = key[s];
    if (k == LPA_EMPTY)
      continue;
    const int32_t c = sum[s];
    if (k == self.cur)
      own = c;
    if (D::own_competes || k != self.cur)
      D::template consider<NARROW>(st, self, k, c, mine, mine_tie);
  }
  unsigned long long best = mine;
#pragma unroll
  for (int d = G / 2; d > 0; d >>= 1) {
    const unsigned long long other = __shfl_xor(best, d, G);
    best = other > best ? other : best;
    own = max(own, __shfl_xor(own, d, G));
  }
  typename D::tie_t tie = mine == best ? mine_tie : D::no_tie;
#pragma unroll
  for (int d = G / 2; d > 0; d >>= 1)
    tie = D::first_tie(tie, __shfl_xor(tie, d, G));
  D::template decided<NARROW, G>(st, v, lo, hi, l, self, own, best, D::label_of(tie), tally);
}

/// The rows rows[0, n_rows) of one class, G lanes each.
template <class D, int G>
inline __global__ void __launch_bounds__(LPA_BLOCK)
    sweep_group_kernel(typename D::state_t st, const int32_t* rows, int32_t n_rows, typename D::counters_t* ctr) {
  static_assert(G == LPA_SMALL || G == wave_size, "a group is 8 lanes or a wavefront");
  constexpr int SLOTS = G == LPA_SMALL ? LPA_SMALL_SLOTS : LPA_WAVE_SLOTS;
  constexpr int GROUPS = LPA_BLOCK / G;
  __shared__ int32_t s_key[GROUPS * SLOTS], s_sum[GROUPS * SLOTS];
  const int l = threadIdx.x % G;
  const int group = threadIdx.x / G;
  typename D::tally_t tally{};
  for (int64_t r0 = (int64_t)blockIdx.x * GROUPS; r0 < n_rows; r0 += (int64_t)gridDim.x * GROUPS) {
    const int64_t r = r0 + group;
    sweep_group_decide<D, G, SLOTS, false>(st, r < n_rows ? rows[r] : -1, s_key + group * SLOTS, s_sum + group * SLOTS, l,
                                           tally);
  }
  D::template flush<false>(tally, ctr);
}

/// LDS words of a workgroup's decision.
template <class D>
struct sweep_lds_t {
  unsigned long long best;
  typename D::tie_t tie;
  int own, fresh, overflow;
};

/**
 * @brief The labels of row v = entries [lo, hi) summed by the workgroup into key/sum[0, cap).
 * True when the row has more distinct labels than cap / 2, or an insert found no slot: the table
 * is then of no use.  Every thread calls it; the words of `s` are set for sweep_block_pick.
 * GLOBAL: the cleared table is at the device's level before any atomic finds it, and the sums are
 * before the scan reads them (two fences; the path is taken only by rows that overflowed).
 */
template <class D, int BLOCK, bool GLOBAL, bool NARROW>
__device__ __forceinline__ bool sweep_count(const typename D::state_t& st, int32_t v, int32_t lo, int32_t hi,
                                            int32_t* key, int32_t* sum, unsigned cap, sweep_lds_t<D>& s) {
  const int tid = threadIdx.x;
  for (unsigned i = tid; i < cap; i += BLOCK) {
    lpa_store<GLOBAL>(key + i, LPA_EMPTY);
    lpa_store<GLOBAL>(sum + i, 0);
  }
  if (tid == 0) {
    s.best = 0;
    s.tie = D::no_tie;
    s.own = 0;
    s.fresh = 0;
    s.overflow = 0;
  }
  if (GLOBAL)
    __threadfence();
  __syncthreads();
  constexpr int AHEAD = 4;  // labels gathered before the first insert: their loads overlap
  for (int64_t e0 = (int64_t)lo + tid; e0 < hi; e0 += (int64_t)AHEAD * BLOCK) {
    int32_t c[AHEAD], w[AHEAD];
#pragma unroll
    for (int j = 0; j < AHEAD; ++j) {
      const int64_t e = e0 + (int64_t)j * BLOCK;
      const int32_t u = e < hi ? st.aj[e] : v;  // past the row: skipped like a self entry
      c[j] = u != v ? lpa_load<NARROW>(st.label + u) : LPA_EMPTY;
      w[j] = u != v ? D::weight(st, e) : 1;
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

/// The decision of vertex v from the summed table; every thread calls it, after sweep_count
/// returned false.  Its last barrier frees `s`; the table is free when every thread has returned.
template <class D, int BLOCK, bool GLOBAL, bool NARROW>
__device__ __forceinline__ void sweep_block_pick(const typename D::state_t& st, int32_t v, int32_t lo, int32_t hi,
                                                 const int32_t* key, const int32_t* sum, unsigned cap, sweep_lds_t<D>& s,
                                                 typename D::tally_t& tally) {
  const int tid = threadIdx.x;
  const typename D::self_t self = D::template self<NARROW>(st, v);
  unsigned long long mine = 0;
  typename D::tie_t mine_tie = D::no_tie;
  for (unsigned i = tid; i < cap; i += BLOCK) {
    const int32_t k = lpa_load<GLOBAL>(key + i);
    if (k == LPA_EMPTY)
      continue;
    const int32_t c = lpa_load<GLOBAL>(sum + i);
    if (k == self.cur)
      s.own = c;  // one slot holds cur
    if (D::own_competes || k != self.cur)
      D::template consider<NARROW>(st, self, k, c, mine, mine_tie);
  }
  const unsigned long long wave_best = wave_max(mine);
  if (lane_id() == 0 && wave_best)
    atomicMax(&s.best, wave_best);
  __syncthreads();
  if (mine && mine == s.best)
    D::offer(&s.tie, mine_tie);
  __syncthreads();
  const unsigned long long best = s.best;
  const typename D::tie_t tie = s.tie;
  const int32_t own = s.own;
  __syncthreads();  // `s` is read: thread 0 of the next row may set it
  D::template decided<NARROW, BLOCK>(st, v, lo, hi, tid, self, own, best, D::label_of(tie), tally);
}

/**
 * @brief A workgroup per row of rows[0, n_rows), the table in dynamic LDS: `max_slots` keys, then
 * as many sums.  A row that overflows goes to over[] as (unit of its table in the pool << 32) | v,
 * undecided; the pool gives it 4 words per entry.
 */
template <class D, int BLOCK>
inline __global__ void __launch_bounds__(BLOCK)
    sweep_block_kernel(typename D::state_t st, const int32_t* rows, int32_t n_rows, int32_t max_slots,
                       unsigned long long* over, typename D::counters_t* ctr) {
  extern __shared__ int32_t s_dyn[];
  __shared__ sweep_lds_t<D> s;
  typename D::tally_t tally{};
  for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const int32_t v = rows[r];
    if (!D::template wants<false>(st, v))  // uniform; what it reads changes behind the barriers of the count
      continue;
    const int32_t lo = st.ap[v], hi = st.ap[v + 1];
    const unsigned cap = lpa_slots_for(hi - lo, max_slots);
    if (sweep_count<D, BLOCK, false, false>(st, v, lo, hi, s_dyn, s_dyn + max_slots, cap, s)) {
      if (threadIdx.x == 0) {
        const int at = atomicAdd(&ctr->pool_at, hi - lo);
        over[atomicAdd(&ctr->overflow_n, 1)] = ((unsigned long long)(unsigned)at << 32) | (unsigned)v;
      }
      __syncthreads();  // `s` is read
      continue;
    }
    sweep_block_pick<D, BLOCK, false, false>(st, v, lo, hi, s_dyn, s_dyn + max_slots, cap, s, tally);
  }
  D::template flush<false>(tally, ctr);
}

/// The rows on the overflow list, a workgroup each, with a table of two slots per entry in the pool.
template <class D>
inline __global__ void __launch_bounds__(LPA_BIG_BLOCK)
    sweep_fallback_kernel(typename D::state_t st, const unsigned long long* over, int32_t* pool,
                          typename D::counters_t* ctr) {
  __shared__ sweep_lds_t<D> s;
  const int32_t items = ctr->overflow_n;  // written by the kernel before this one; constant here
  typename D::tally_t tally{};
  for (int32_t i = blockIdx.x; i < items; i += gridDim.x) {
    const unsigned long long item = over[i];
    const int32_t v = (int32_t)(item & 0xffffffffu);
    const int32_t lo = st.ap[v], hi = st.ap[v + 1];
    const unsigned cap = 2u * (unsigned)(hi - lo);
    int32_t* key = pool + 4 * (std::size_t)(item >> 32);
    // two slots per entry: the table cannot overflow
    sweep_count<D, LPA_BIG_BLOCK, true, false>(st, v, lo, hi, key, key + cap, cap, s);
    sweep_block_pick<D, LPA_BIG_BLOCK, true, false>(st, v, lo, hi, key, key + cap, cap, s, tally);
  }
  D::template flush<false>(tally, ctr);
}

/**
 * @brief ONE workgroup: the classes [c0, c1), each of at most LPA_NARROW_VERTICES vertices, with a
 * barrier between them.  order[starts[4 c + b] .. starts[4 c + b + 1]) are the rows of bin b of
 * class c.  Dynamic LDS: max(16 wavefront tables, 2 * max_slots) words.  pool: 4 words per entry of
 * the longest row of bins 2 and 3.
 */
template <class D>
inline __global__ void __launch_bounds__(LPA_BIG_BLOCK)
    sweep_narrow_kernel(typename D::state_t st, const int32_t* order, const int32_t* starts, int32_t c0, int32_t c1,
                        int32_t max_slots, int32_t* pool, typename D::counters_t* ctr) {
  constexpr int WAVES = LPA_BIG_BLOCK / wave_size;
  extern __shared__ int32_t s_dyn[];
  __shared__ sweep_lds_t<D> s;
  const int lane = lane_id();
  const int wave = threadIdx.x / wave_size;
  typename D::tally_t tally{};
  for (int32_t c = c0; c < c1; ++c) {
    const int32_t b0 = starts[LPA_BINS * c], b2 = starts[LPA_BINS * c + 2], b4 = starts[LPA_BINS * c + LPA_BINS];
    for (int32_t r0 = b0; r0 < b2; r0 += WAVES) {
      const int32_t r = r0 + wave;
      sweep_group_decide<D, wave_size, LPA_WAVE_SLOTS, true>(st, r < b2 ? order[r] : -1,
                                                             s_dyn + wave * 2 * LPA_WAVE_SLOTS,
                                                             s_dyn + wave * 2 * LPA_WAVE_SLOTS + LPA_WAVE_SLOTS, lane,
                                                             tally);
    }
    __syncthreads();  // the tables are the workgroup's now
    for (int32_t r = b2; r < b4; ++r) {
      const int32_t v = order[r];
      if (!D::template wants<true>(st, v))
        continue;
      const int32_t lo = st.ap[v], hi = st.ap[v + 1];
      unsigned cap = lpa_slots_for(hi - lo, max_slots);
      int32_t *key = s_dyn, *sum = s_dyn + max_slots;
      if (sweep_count<D, LPA_BIG_BLOCK, false, true>(st, v, lo, hi, key, sum, cap, s)) {
        __syncthreads();  // `s` is read
        cap = 2u * (unsigned)(hi - lo);
        key = pool;
        sum = pool + cap;
        sweep_count<D, LPA_BIG_BLOCK, true, true>(st, v, lo, hi, key, sum, cap, s);
        sweep_block_pick<D, LPA_BIG_BLOCK, true, true>(st, v, lo, hi, key, sum, cap, s, tally);
      } else {
        sweep_block_pick<D, LPA_BIG_BLOCK, false, true>(st, v, lo, hi, key, sum, cap, s, tally);
      }
    }
    D::class_done(st, order, b0, b4, tally);
    __syncthreads();  // the class is decided: what it wrote is the next one's input
  }
  D::template flush<true>(tally, ctr);
}

/// first[l] = the smallest vertex labelled l (first[] starts as all ones).  A wavefront whose
/// vertices share a label sends one minimum, and nobody sends what the word already beats: the
/// final labels of an R-MAT are one giant community, and its word takes ~90 atomics per microsecond.
inline __global__ void __launch_bounds__(LPA_BLOCK) lpa_first_kernel(const int32_t* label, int32_t n, unsigned* first) {
  const int lane = lane_id();
  const int64_t stride = (int64_t)gridDim.x * LPA_BLOCK;
  for (int64_t v0 = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x - lane; v0 < n; v0 += stride) {
    const int64_t v = v0 + lane;
    const int32_t l = v < n ? label[v] : -1;
    const int32_t l0 = __shfl(l, 0, wave_size);
    if (__all(l == l0)) {  // a whole wavefront inside n: lane 0 holds the smallest id
      if (lane == 0 && load_relaxed(first + l0) > (unsigned)v)
        atomicMin(&first[l0], (unsigned)v);
    } else if (v < n && load_relaxed(first + l) > (unsigned)v) {
      atomicMin(&first[l], (unsigned)v);
    }
  }
}

/// inside += the weight of the entries (v, u) with label[v] == label[u] (aw is not read unless
/// WEIGHTED: every entry weighs 1): chunks of LPA_BLOCK rows flattened over the workgroup.  Rows
/// above LPA_INSIDE_SEGMENT entries go to the big list in segments ...
template <bool WEIGHTED, class counters_t>
inline __global__ void __launch_bounds__(LPA_BLOCK)
    sweep_inside_kernel(const int32_t* ap, const int32_t* aj, const int32_t* aw, const int32_t* label, int32_t n,
                        int2* big, counters_t* ctr) {
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

/// ... which the grid walks a workgroup per segment: no launch is as long as its longest row.
template <bool WEIGHTED, class counters_t>
inline __global__ void __launch_bounds__(LPA_BLOCK)
    sweep_inside_big_kernel(const int32_t* ap, const int32_t* aj, const int32_t* aw, const int32_t* label,
                            const int2* big, counters_t* ctr) {
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

/// squares += tot[l]^2 in 64 bits (tot[l] is at most the entries < 2^31: the sum is below 2^62).
template <class tot_t, class counters_t>
inline __global__ void __launch_bounds__(LPA_BLOCK) sweep_squares_kernel(const tot_t* tot, int32_t n, counters_t* ctr) {
  unsigned long long sum = 0;
  for (int64_t l = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; l < n; l += (int64_t)gridDim.x * LPA_BLOCK) {
    const unsigned long long t = (unsigned long long)tot[l];
    sum += t * t;
  }
  sum = wave_sum(sum);
  if (lane_id() == 0 && sum)
    atomicAdd(&ctr->squares, sum);
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

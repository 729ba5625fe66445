/**
 * @file lpa_kernels.hxx
 * @brief Community detection (grx_lpa): semi-synchronous label propagation (Cordasco, Gargano 2010)
 * over the colour classes of grx_color, and the modularity of a labelling (grx_modularity).
 *
 * A sweep takes the colour classes in order; the vertices of a class are never adjacent, so they
 * decide at once from the labels as they stand.  A decision is the most frequent label over the
 * row's entries other than self loops: every entry costs one gather of label[u] and one insert into
 * a table of (label, count) -- open addressing, atomicCAS on the key, atomicAdd on the count, at most
 * half full.  The vertex keeps its label when that is among the maxima and takes the maximum of
 * smallest fmix32(label) otherwise.  Counts are integers, so the answer does not depend on the
 * order of the inserts.
 *
 *   lpa_init_kernel            label[v] = v, dirty[v] = 1.
 *   lpa_starts_kernel          first position of every (class, bin) key in the sorted keys.
 *   lpa_entries_kernel         row entries per (class, bin).
 *   lpa_group_kernel<G>        a class's rows of one bin, G lanes per row: 8 lanes and 64 slots for
 *                              short rows, a wavefront and 512 slots up to 256 entries; static LDS.
 *   lpa_block_kernel<BLOCK>    a workgroup per row, the table in dynamic LDS, two slots per entry
 *                              up to `max_slots`.  A row with more distinct labels than half the
 *                              table overflows and goes to a list ...
 *   lpa_fallback_kernel        ... whose rows get a table of two slots per entry in global memory:
 *                              the same inserts with agent-scope accesses, a workgroup per row.
 *   lpa_narrow_kernel          ONE workgroup runs consecutive small classes with a barrier between
 *                              them: a wavefront per row up to 256 entries, the workgroup per row
 *                              above, the global table in place when the LDS table overflows.
 *   lpa_publish_kernel         the sweep's hand-off: the change count and the entries read.
 *   lpa_first_kernel, lpa_canonical_kernel   the smallest vertex id per final label, and the
 *                              communities counted.
 *   lpa_range_kernel, lpa_tot_kernel, lpa_inside_kernel, lpa_inside_big_kernel, lpa_squares_kernel
 *                              modularity in integers.
 *
 * Dirty flags, a byte per vertex: a vertex decides only while its flag is set and clears it; a
 * vertex that changes its label sets the flag of every other vertex in its row.  A vertex none of
 * whose neighbours changed since its last decision would decide the same.  Within a launch the
 * flags set belong to other classes and the flags cleared to this one, and labels are read of
 * other classes and written of this one: nothing is handed between workgroups inside a launch.
 * The one-workgroup kernel does hand labels and flags from class to class; there they are read and
 * written with agent-scope relaxed accesses behind the workgroup's barrier.
 *
 * The kernels are `inline`: capi_lpa.hip and capi_louvain.hip (through louvain_kernels.hxx, which
 * shares the schedule, the table and the first-occurrence pass) both include this header.
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
constexpr int LPA_INSIDE_SEGMENT = 4096;  // modularity: longer rows are cut into segments of this many entries
constexpr int32_t LPA_EMPTY = -1;

/// Device counters of one call.
struct lpa_counters_t {
  unsigned long long changes;      // labels changed in the sweep that runs
  unsigned long long read;         // row entries read by decisions and by marking, the whole call
  unsigned long long communities;  // vertices that are their label's smallest member
  unsigned long long inside;       // modularity: entries whose ends share a label
  unsigned long long squares;      // modularity: sum of tot(l)^2
  int overflow_n;                  // rows on the overflow list of the class that runs
  int pool_at;                     // ... and the units of 4 words their tables take
  int bad;                         // modularity: a label outside [0, V)
  int big_n;                       // modularity: segments on the big list
};
/// What the host reads at a hand-off (words of the pinned mirror).
enum { LPA_CHANGES = 0, LPA_READ, LPA_COMMUNITIES, LPA_INSIDE, LPA_SQUARES, LPA_BAD, LPA_WORDS };

/// What every decision reads and writes.  dirty == nullptr: every vertex decides every sweep.
struct lpa_state_t {
  const int32_t* ap;
  const int32_t* aj;
  int32_t* label;
  unsigned char* dirty;
};

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

/// Larger for the larger count, then for the smaller fmix32(label); 0 is below every entry's rank.
__device__ __forceinline__ unsigned long long lpa_rank(int32_t count, int32_t label) {
  return ((unsigned long long)(unsigned)count << 32) | (0xffffffffu - fmix32((unsigned)label));
}

/// Count label l in the table key/cnt[0, cap), `w` times (grx_louvain adds an entry's weight):
/// `fresh` += 1 when this call took a slot.  False when `cap` probes found neither l nor an empty
/// slot.  GLOBAL: the table is in global memory.
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

inline __global__ void __launch_bounds__(LPA_BLOCK) lpa_init_kernel(int32_t* label, unsigned char* dirty, int32_t n) {
  for (int64_t v = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * LPA_BLOCK) {
    label[v] = (int32_t)v;
    if (dirty)
      dirty[v] = 1;
  }
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

/// Add what the lanes of a kernel counted.
__device__ __forceinline__ void lpa_flush(unsigned long long read, unsigned long long changed, lpa_counters_t* ctr) {
  read = wave_sum(read);
  changed = wave_sum(changed);
  if (lane_id() == 0) {
    if (read)
      atomicAdd(&ctr->read, read);
    if (changed)
      atomicAdd(&ctr->changes, changed);
  }
}

/**
 * @brief The decision of vertex v (-1: none) by the G lanes of a group, lane l, with the group's
 * table key/cnt[0, SLOTS) in LDS; a row has at most SLOTS / 2 entries.  G lanes are part of one
 * wavefront, and every thread of the workgroup calls this the same number of times (two barriers).
 */
template <int G, int SLOTS, bool NARROW>
__device__ __forceinline__ void lpa_group_decide(const lpa_state_t& st, int32_t v, int32_t* key, int32_t* cnt, int l,
                                                 unsigned long long& read, unsigned long long& changed) {
  int32_t lo = 0, hi = 0;
  if (v >= 0 && (!st.dirty || lpa_load<NARROW>(st.dirty + v))) {
    lo = st.ap[v];
    hi = st.ap[v + 1];
  }
  for (int s = l; s < SLOTS; s += G) {
    key[s] = LPA_EMPTY;
    cnt[s] = 0;
  }
  __syncthreads();
  int fresh = 0;
  for (int32_t e = lo + l; e < hi; e += G) {
    const int32_t u = st.aj[e];
    if (u != v)
      lpa_insert<false>(key, cnt, SLOTS, lpa_load<NARROW>(st.label + u), fresh);
  }
  __syncthreads();
  if (hi == lo)  // uniform in the group
    return;
  const int32_t cur = lpa_load<NARROW>(st.label + v);
  unsigned long long mine = 0;
  int32_t mine_label = -1, cur_count = 0;
  for (int s = l; s < SLOTS; s += G) {
    const int32_t k = key[s];
    if (k == LPA_EMPTY)
      continue;
    const int32_t c = cnt[s];
    const unsigned long long r = lpa_rank(c, k);
    if (r > mine) {
      mine = r;
      mine_label = k;
    }
    if (k == cur)
      cur_count = c;
  }
  unsigned long long best = mine;
#pragma unroll
  for (int d = G / 2; d > 0; d >>= 1) {
    const unsigned long long other = __shfl_xor(best, d, G);
    best = other > best ? other : best;
    cur_count = max(cur_count, __shfl_xor(cur_count, d, G));
  }
  int32_t lab = mine == best ? mine_label : -1;  // fmix32 is a bijection: one slot has this rank
#pragma unroll
  for (int d = G / 2; d > 0; d >>= 1)
    lab = max(lab, __shfl_xor(lab, d, G));
  const bool move = best != 0 && (int32_t)(best >> 32) != cur_count;
  if (l == 0) {
    read += (unsigned long long)(hi - lo);
    if (st.dirty)
      lpa_store<NARROW>(st.dirty + v, (unsigned char)0);
    if (move) {
      lpa_store<NARROW>(st.label + v, lab);
      ++changed;
      if (st.dirty)
        read += (unsigned long long)(hi - lo);
    }
  }
  if (move && st.dirty)
    for (int32_t e = lo + l; e < hi; e += G) {
      const int32_t u = st.aj[e];
      if (u != v)
        lpa_store<NARROW>(st.dirty + u, (unsigned char)1);
    }
}

/// The rows rows[0, n_rows) of one class, G lanes each.
template <int G>
inline __global__ void __launch_bounds__(LPA_BLOCK)
    lpa_group_kernel(lpa_state_t st, const int32_t* rows, int32_t n_rows, lpa_counters_t* ctr) {
  static_assert(G == LPA_SMALL || G == wave_size, "a group is 8 lanes or a wavefront");
  constexpr int SLOTS = G == LPA_SMALL ? LPA_SMALL_SLOTS : LPA_WAVE_SLOTS;
  constexpr int GROUPS = LPA_BLOCK / G;
  __shared__ int32_t s_key[GROUPS * SLOTS], s_cnt[GROUPS * SLOTS];
  const int l = threadIdx.x % G;
  const int group = threadIdx.x / G;
  unsigned long long read = 0, changed = 0;
  for (int64_t r0 = (int64_t)blockIdx.x * GROUPS; r0 < n_rows; r0 += (int64_t)gridDim.x * GROUPS) {
    const int64_t r = r0 + group;
    lpa_group_decide<G, SLOTS, false>(st, r < n_rows ? rows[r] : -1, s_key + group * SLOTS, s_cnt + group * SLOTS, l,
                                      read, changed);
  }
  lpa_flush(read, changed, ctr);
}

/// LDS words of a workgroup's decision.
struct lpa_block_lds_t {
  unsigned long long best;
  int cur, label, fresh, overflow;
};

/**
 * @brief The labels of row v = entries [lo, hi) counted by the workgroup into key/cnt[0, cap).
 * True when the row has more distinct labels than cap / 2, or an insert found no slot: the table
 * is then of no use.  Every thread calls it; the words of `s` are set for lpa_block_pick.
 */
template <int BLOCK, bool GLOBAL, bool NARROW>
__device__ __forceinline__ bool lpa_block_count(const lpa_state_t& st, int32_t v, int32_t lo, int32_t hi, int32_t* key,
                                                int32_t* cnt, unsigned cap, lpa_block_lds_t& s) {
  const int tid = threadIdx.x;
  for (unsigned i = tid; i < cap; i += BLOCK) {
    lpa_store<GLOBAL>(key + i, LPA_EMPTY);
    lpa_store<GLOBAL>(cnt + i, 0);
  }
  if (tid == 0) {
    s.best = 0;
    s.cur = 0;
    s.label = -1;
    s.fresh = 0;
    s.overflow = 0;
  }
  __syncthreads();
  constexpr int AHEAD = 4;  // labels gathered before the first insert: their loads overlap
  for (int64_t e0 = (int64_t)lo + tid; e0 < hi; e0 += (int64_t)AHEAD * BLOCK) {
    int32_t l[AHEAD];
#pragma unroll
    for (int j = 0; j < AHEAD; ++j) {
      const int64_t e = e0 + (int64_t)j * BLOCK;
      const int32_t u = e < hi ? st.aj[e] : v;  // past the row: skipped like a self loop
      l[j] = u != v ? lpa_load<NARROW>(st.label + u) : LPA_EMPTY;
    }
    if (__hip_atomic_load(&s.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
      break;
    bool full = false;
#pragma unroll
    for (int j = 0; j < AHEAD; ++j) {
      if (l[j] == LPA_EMPTY || full)
        continue;
      int fresh = 0;
      full = !lpa_insert<GLOBAL>(key, cnt, cap, l[j], fresh) || (fresh && (unsigned)atomicAdd(&s.fresh, 1) >= cap / 2);
    }
    if (full) {
      __hip_atomic_store(&s.overflow, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      break;
    }
  }
  __syncthreads();
  return s.overflow != 0;
}

/// The decision of vertex v from the counted table; every thread calls it, after lpa_block_count
/// returned false.  Ends with a barrier: the table and `s` are then free.
template <int BLOCK, bool GLOBAL, bool NARROW>
__device__ __forceinline__ void lpa_block_pick(const lpa_state_t& st, int32_t v, int32_t lo, int32_t hi,
                                               const int32_t* key, const int32_t* cnt, unsigned cap, lpa_block_lds_t& s,
                                               unsigned long long& read, unsigned long long& changed) {
  const int tid = threadIdx.x;
  const int32_t cur = lpa_load<NARROW>(st.label + v);
  unsigned long long mine = 0;
  int32_t mine_label = -1;
  for (unsigned i = tid; i < cap; i += BLOCK) {
    const int32_t k = lpa_load<GLOBAL>(key + i);
    if (k == LPA_EMPTY)
      continue;
    const int32_t c = lpa_load<GLOBAL>(cnt + i);
    const unsigned long long r = lpa_rank(c, k);
    if (r > mine) {
      mine = r;
      mine_label = k;
    }
    if (k == cur)
      s.cur = c;  // one slot holds cur
  }
  const unsigned long long wave_best = wave_max(mine);
  if (lane_id() == 0 && wave_best)
    atomicMax(&s.best, wave_best);
  __syncthreads();
  if (mine && mine == s.best)
    s.label = mine_label;  // one slot has this rank
  __syncthreads();
  const unsigned long long best = s.best;
  const int32_t lab = s.label;
  const bool move = best != 0 && (int32_t)(best >> 32) != s.cur;
  __syncthreads();  // `s` is read: thread 0 of the next row may set it
  if (tid == 0) {
    read += (unsigned long long)(hi - lo);
    if (st.dirty)
      lpa_store<NARROW>(st.dirty + v, (unsigned char)0);
    if (move) {
      lpa_store<NARROW>(st.label + v, lab);
      ++changed;
      if (st.dirty)
        read += (unsigned long long)(hi - lo);
    }
  }
  if (move && st.dirty)
    for (int32_t e = lo + tid; e < hi; e += BLOCK) {
      const int32_t u = st.aj[e];
      if (u != v)
        lpa_store<NARROW>(st.dirty + u, (unsigned char)1);
    }
}

/// Slots of the LDS table of a row of `len` entries: two per entry, within [LPA_MIN_SLOTS, max_slots].
__host__ __device__ __forceinline__ unsigned lpa_slots_for(int32_t len, int32_t max_slots) {
  const long long want = 2ll * len;
  return (unsigned)(want < LPA_MIN_SLOTS ? LPA_MIN_SLOTS : want > max_slots ? max_slots : want);
}

/**
 * @brief A workgroup per row of rows[0, n_rows), the table in dynamic LDS: `max_slots` keys, then
 * as many counts.  A row that overflows goes to over[] as (unit of its table in the pool << 32) | v,
 * its flag still set; the pool gives it 4 words per entry.
 */
template <int BLOCK>
inline __global__ void __launch_bounds__(BLOCK)
    lpa_block_kernel(lpa_state_t st, const int32_t* rows, int32_t n_rows, int32_t max_slots, unsigned long long* over,
                     lpa_counters_t* ctr) {
  extern __shared__ int32_t s_dyn[];
  __shared__ lpa_block_lds_t s;
  unsigned long long read = 0, changed = 0;
  for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const int32_t v = rows[r];
    if (st.dirty && !st.dirty[v])  // uniform; the flag is cleared behind the barriers of the count
      continue;
    const int32_t lo = st.ap[v], hi = st.ap[v + 1];
    const unsigned cap = lpa_slots_for(hi - lo, max_slots);
    if (lpa_block_count<BLOCK, false, false>(st, v, lo, hi, s_dyn, s_dyn + max_slots, cap, s)) {
      if (threadIdx.x == 0) {
        const int at = atomicAdd(&ctr->pool_at, hi - lo);
        over[atomicAdd(&ctr->overflow_n, 1)] = ((unsigned long long)(unsigned)at << 32) | (unsigned)v;
      }
      __syncthreads();  // `s` is read
      continue;
    }
    lpa_block_pick<BLOCK, false, false>(st, v, lo, hi, s_dyn, s_dyn + max_slots, cap, s, read, changed);
  }
  lpa_flush(read, changed, ctr);
}

/// The rows on the overflow list, a workgroup each, with a table of two slots per entry in the pool.
inline __global__ void __launch_bounds__(LPA_BIG_BLOCK)
    lpa_fallback_kernel(lpa_state_t st, const unsigned long long* over, int32_t* pool, lpa_counters_t* ctr) {
  __shared__ lpa_block_lds_t s;
  const int32_t items = ctr->overflow_n;  // written by the kernel before this one; constant here
  unsigned long long read = 0, changed = 0;
  for (int32_t i = blockIdx.x; i < items; i += gridDim.x) {
    const unsigned long long item = over[i];
    const int32_t v = (int32_t)(item & 0xffffffffu);
    const int32_t lo = st.ap[v], hi = st.ap[v + 1];
    const unsigned cap = 2u * (unsigned)(hi - lo);
    int32_t* key = pool + 4 * (std::size_t)(item >> 32);
    // two slots per entry: the count cannot overflow
    lpa_block_count<LPA_BIG_BLOCK, true, false>(st, v, lo, hi, key, key + cap, cap, s);
    lpa_block_pick<LPA_BIG_BLOCK, true, false>(st, v, lo, hi, key, key + cap, cap, s, read, changed);
  }
  lpa_flush(read, changed, ctr);
}

/**
 * @brief ONE workgroup: the classes [c0, c1), each of at most LPA_NARROW_VERTICES vertices, with a
 * barrier between them.  order[starts[4 c + b] .. starts[4 c + b + 1]) are the rows of bin b of
 * class c.  Dynamic LDS: max(16 wavefront tables, 2 * max_slots) words.  pool: 4 words per entry of
 * the longest row of bins 2 and 3.
 */
inline __global__ void __launch_bounds__(LPA_BIG_BLOCK)
    lpa_narrow_kernel(lpa_state_t st, const int32_t* order, const int32_t* starts, int32_t c0, int32_t c1,
                      int32_t max_slots, int32_t* pool, lpa_counters_t* ctr) {
  constexpr int WAVES = LPA_BIG_BLOCK / wave_size;
  extern __shared__ int32_t s_dyn[];
  __shared__ lpa_block_lds_t s;
  const int lane = lane_id();
  const int wave = threadIdx.x / wave_size;
  unsigned long long read = 0, changed = 0;
  for (int32_t c = c0; c < c1; ++c) {
    const int32_t b0 = starts[LPA_BINS * c], b2 = starts[LPA_BINS * c + 2], b4 = starts[LPA_BINS * c + LPA_BINS];
    for (int32_t r0 = b0; r0 < b2; r0 += WAVES) {
      const int32_t r = r0 + wave;
      lpa_group_decide<wave_size, LPA_WAVE_SLOTS, true>(st, r < b2 ? order[r] : -1, s_dyn + wave * 2 * LPA_WAVE_SLOTS,
                                                        s_dyn + wave * 2 * LPA_WAVE_SLOTS + LPA_WAVE_SLOTS, lane, read,
                                                        changed);
    }
    __syncthreads();  // the tables are the workgroup's now
    for (int32_t r = b2; r < b4; ++r) {
      const int32_t v = order[r];
      if (st.dirty && !load_relaxed(st.dirty + v))
        continue;
      const int32_t lo = st.ap[v], hi = st.ap[v + 1];
      unsigned cap = lpa_slots_for(hi - lo, max_slots);
      int32_t *key = s_dyn, *cnt = s_dyn + max_slots;
      if (lpa_block_count<LPA_BIG_BLOCK, false, true>(st, v, lo, hi, key, cnt, cap, s)) {
        __syncthreads();  // `s` is read
        cap = 2u * (unsigned)(hi - lo);
        key = pool;
        cnt = pool + cap;
        lpa_block_count<LPA_BIG_BLOCK, true, true>(st, v, lo, hi, key, cnt, cap, s);
        lpa_block_pick<LPA_BIG_BLOCK, true, true>(st, v, lo, hi, key, cnt, cap, s, read, changed);
      } else {
        lpa_block_pick<LPA_BIG_BLOCK, false, true>(st, v, lo, hi, key, cnt, cap, s, read, changed);
      }
    }
    __syncthreads();  // the class is decided: its labels and flags are the next one's input
  }
  lpa_flush(read, changed, ctr);
}

/// The hand-off that ends a sweep: the sweep's changes (cleared for the next) and the entries read.
inline __global__ void lpa_publish_kernel(lpa_counters_t* ctr, unsigned long long* mirror, int sequence_slot,
                                   unsigned long long sequence) {
  if (threadIdx.x == 0) {
    mirror[LPA_CHANGES] = ctr->changes;
    mirror[LPA_READ] = ctr->read;
    mirror[LPA_COMMUNITIES] = ctr->communities;
    mirror[LPA_INSIDE] = ctr->inside;
    mirror[LPA_SQUARES] = ctr->squares;
    mirror[LPA_BAD] = (unsigned long long)ctr->bad;
    ctr->changes = 0;
    stamp_handoff(mirror, sequence_slot, sequence);
  }
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

/// label[v] = first[label[v]], in place; the vertices that are their own community's name are counted.
inline __global__ void __launch_bounds__(LPA_BLOCK)
    lpa_canonical_kernel(int32_t* label, int32_t n, const unsigned* first, lpa_counters_t* ctr) {
  unsigned long long mine = 0;
  for (int64_t v = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * LPA_BLOCK) {
    const int32_t name = (int32_t)first[label[v]];
    label[v] = name;
    mine += name == (int32_t)v;
  }
  mine = wave_sum(mine);
  if (lane_id() == 0 && mine)
    atomicAdd(&ctr->communities, mine);
}

/// bad = 1 when a label is outside [0, n).
inline __global__ void __launch_bounds__(LPA_BLOCK) lpa_range_kernel(const int32_t* label, int32_t n, lpa_counters_t* ctr) {
  bool bad = false;
  for (int64_t v = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * LPA_BLOCK) {
    const int32_t l = label[v];
    bad |= l < 0 || l >= n;
  }
  if (bad)
    atomicOr(&ctr->bad, 1);
}

/// tot[l] += the row lengths of the vertices labelled l (at most nnz < 2^31 each); the lanes of a
/// wavefront that share a label add once.
inline __global__ void __launch_bounds__(LPA_BLOCK)
    lpa_tot_kernel(const int32_t* ap, const int32_t* label, int32_t n, unsigned* tot) {
  const int lane = lane_id();
  const int64_t stride = (int64_t)gridDim.x * LPA_BLOCK;
  for (int64_t v0 = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x - lane; v0 < n; v0 += stride) {
    const int64_t v = v0 + lane;
    int32_t l = -1;
    unsigned d = 0;
    if (v < n) {
      l = label[v];
      d = (unsigned)(ap[v + 1] - ap[v]);
      if (l < 0 || l >= n)  // lpa_range_kernel reports it; nothing is added out of bounds
        l = -1;
    }
    // twice: the lanes that share the first pending lane's label add once; the rest add alone
    bool pending = l >= 0 && d;
    for (int round = 0; round < 2; ++round) {
      const unsigned long long todo = __ballot(pending);
      if (!todo)  // uniform
        break;
      const int leader = __ffsll((long long)todo) - 1;
      const int32_t shared = __shfl(l, leader, wave_size);
      const bool same = pending && l == shared;
      const unsigned sum = wave_sum(same ? d : 0u);
      if (lane == leader)
        atomicAdd(&tot[shared], sum);
      pending = pending && !same;
    }
    if (pending)
      atomicAdd(&tot[l], d);
  }
}

/// inside += the entries (v, u) with label[v] == label[u]: chunks of LPA_BLOCK rows flattened over
/// the workgroup.  Rows above LPA_INSIDE_SEGMENT entries go to the big list in segments ...
inline __global__ void __launch_bounds__(LPA_BLOCK)
    lpa_inside_kernel(const int32_t* ap, const int32_t* aj, const int32_t* label, int32_t n, int2* big,
                      lpa_counters_t* ctr) {
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
    flat_walk<LPA_BLOCK>(d, lo, s_pre, s_base, s_wave,
                         [&](int o, int32_t e) { inside += label[aj[e]] == s_label[o]; });
    __syncthreads();  // s_label is the next chunk's
  }
  inside = wave_sum(inside);
  if (lane_id() == 0 && inside)
    atomicAdd(&ctr->inside, inside);
}

/// ... which the grid walks a workgroup per segment: no launch is as long as its longest row.
inline __global__ void __launch_bounds__(LPA_BLOCK)
    lpa_inside_big_kernel(const int32_t* ap, const int32_t* aj, const int32_t* label, const int2* big,
                          lpa_counters_t* ctr) {
  const int32_t items = ctr->big_n;  // written by the kernel before this one; constant here
  unsigned long long inside = 0;
  for (int32_t i = blockIdx.x; i < items; i += gridDim.x) {
    const int2 item = big[i];  // {vertex, segment of its row}
    const int64_t lo = (int64_t)ap[item.x] + (int64_t)item.y * LPA_INSIDE_SEGMENT;
    const int64_t hi = min((int64_t)ap[item.x + 1], lo + LPA_INSIDE_SEGMENT);
    const int32_t mine = label[item.x];
    for (int64_t e = lo + threadIdx.x; e < hi; e += LPA_BLOCK)
      inside += label[aj[e]] == mine;
  }
  inside = wave_sum(inside);
  if (lane_id() == 0 && inside)
    atomicAdd(&ctr->inside, inside);
}

/// squares += tot[l]^2 in 64 bits (the sum is at most nnz^2 < 2^62).
inline __global__ void __launch_bounds__(LPA_BLOCK) lpa_squares_kernel(const unsigned* tot, int32_t n, lpa_counters_t* ctr) {
  unsigned long long sum = 0;
  for (int64_t l = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; l < n; l += (int64_t)gridDim.x * LPA_BLOCK) {
    const unsigned long long t = tot[l];
    sum += t * t;
  }
  sum = wave_sum(sum);
  if (lane_id() == 0 && sum)
    atomicAdd(&ctr->squares, sum);
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

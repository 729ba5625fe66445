/**
 * @file louvain_kernels.hxx
 * @brief Community detection by multi-level modularity optimisation (grx_louvain), in exact
 * integers: include/essentials_amd.h states the definition.
 *
 * A level graph is a CSR with int32 weights (level 0: the caller's CSR, weight 1 per entry, no
 * weight array: WEIGHTED = false).  A sweep is the colour-class sweep of class_sweep.hxx -- the
 * schedule, the table of (community, weight sum) and the kernels that decide a class at once --
 * with the decision of this header, louvain_decision_t<WEIGHTED>.
 *
 * A decision reads tot[key] per occupied slot and reduces twice: to the largest int64 gain
 * k_vc * E - k(v) * t(c), then to the smallest fmix32 among the slots at that gain.  The vertex
 * writes label[v] in place when that gain beats its own label's; the vertices of a class are never
 * adjacent, so they read each other's labels only through tot, and tot changes only when the class
 * is done: louvain_apply_kernel (or the one-workgroup kernel behind its barrier) compares label[v]
 * with the copy taken when the sweep began, which is also what an undone sweep restores.
 *
 *   louvain_init_kernel              label[v] = v, tot[v] = k(v); on level 0 k(v) = the row length.
 *   louvain_apply_kernel             the class's moves: tot[old] -= k(v), tot[new] += k(v), counted.
 *   louvain_publish_kernel           the sweep's one hand-off: moves, I, S (the score passes of
 *                                    class_sweep.hxx over the maintained tot).
 *   louvain_flag_kernel, louvain_renumber_kernel, louvain_compose_kernel, louvain_keys_kernel,
 *   louvain_unpack_kernel, louvain_name_kernel
 *                                    aggregation: communities ranked by their smallest member, the
 *                                    entries keyed (rank[label[u]] << 32) | rank[label[v]] for the
 *                                    sort and the reduction by key, the next CSR from the sorted keys.
 */
#pragma once

#include <gunrock/hip/kernels/class_sweep.hxx>

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

/// An int64 gain as an unsigned word of the same order; never 0, since |gain| < 2^62.
__device__ __forceinline__ unsigned long long louvain_ordered(long long gain) {
  return (unsigned long long)gain ^ 0x8000000000000000ull;
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

/// The move of vertex v, whose label is now `to`, applied to tot and counted.
__device__ __forceinline__ void louvain_apply(const louvain_state_t& st, int32_t v, int32_t to, unsigned long long& moved) {
  const int32_t from = st.before[v];
  if (from != to) {
    const int32_t kv = st.k[v];
    atomicSub(&st.tot[from], kv);
    atomicAdd(&st.tot[to], kv);
    ++moved;
  }
}

/// The moves of the vertices rows[0, n_rows) of a decided class, applied to tot and counted.
inline __global__ void __launch_bounds__(LPA_BLOCK)
    louvain_apply_kernel(louvain_state_t st, const int32_t* rows, int32_t n_rows, louvain_counters_t* ctr) {
  unsigned long long moved = 0;
  for (int64_t r = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * LPA_BLOCK) {
    const int32_t v = rows[r];
    louvain_apply(st, v, st.label[v], moved);
  }
  moved = wave_sum(moved);
  if (lane_id() == 0 && moved)
    atomicAdd(&ctr->moves, moved);
}

/// Louvain's decision (class_sweep.hxx says what each member is for).  The score of a slot is the
/// ordered gain of moving v there; the slots at the best gain tie, and the smallest
/// (fmix32(c) << 32) | c among them wins.  v's own slot does not compete: v moves when the best
/// other gain beats that of staying, with v taken out of its own community.  Every vertex decides in
/// every sweep, and nothing follows a decision's write-back but the class's moves reaching tot.
template <bool WEIGHTED>
struct louvain_decision_t {
  using state_t = louvain_state_t;
  using counters_t = louvain_counters_t;
  struct self_t {
    int32_t cur, kv;
  };
  struct tally_t {
    unsigned long long moved;  // the one-workgroup kernel's; louvain_apply_kernel counts the wide classes'
  };
  using tie_t = unsigned long long;
  static constexpr tie_t no_tie = ~0ull;
  static constexpr bool own_competes = false;
  static constexpr auto apply_kernel = &louvain_apply_kernel;

  template <bool NARROW>
  static __device__ __forceinline__ bool wants(const state_t&, int32_t) {
    return true;
  }
  static __device__ __forceinline__ int32_t weight(const state_t& st, int64_t e) { return WEIGHTED ? st.aw[e] : 1; }
  template <bool NARROW>
  static __device__ __forceinline__ self_t self(const state_t& st, int32_t v) {
    return {lpa_load<NARROW>(st.label + v), st.k[v]};
  }
  template <bool NARROW>
  static __device__ __forceinline__ void consider(const state_t& st, const self_t& self, int32_t c, int32_t kvc,
                                                  unsigned long long& gain, tie_t& who) {
    const long long t = lpa_load<NARROW>(st.tot + c);
    const unsigned long long g = louvain_ordered((long long)kvc * st.entries - (long long)self.kv * t);
    const unsigned long long w = ((unsigned long long)fmix32((unsigned)c) << 32) | (unsigned)c;
    if (g > gain || (g == gain && w < who)) {
      gain = g;
      who = w;
    }
  }
  static __device__ __forceinline__ tie_t first_tie(tie_t a, tie_t b) { return b < a ? b : a; }
  static __device__ __forceinline__ void offer(tie_t* word, tie_t who) { atomicMin(word, who); }
  static __device__ __forceinline__ int32_t label_of(tie_t who) { return (int32_t)(who & 0xffffffffu); }
  template <bool NARROW>
  static __device__ __forceinline__ bool moves(const state_t& st, const self_t& self, int32_t own_kvc,
                                               unsigned long long best) {
    if (best == 0)  // no other label in the row
      return false;
    const long long t = (long long)lpa_load<NARROW>(st.tot + self.cur) - self.kv;
    return best > louvain_ordered((long long)own_kvc * st.entries - (long long)self.kv * t);
  }
  /// Thread 0 writes the label when v moves; the move reaches tot when the class is done.
  template <bool NARROW, int WIDTH>
  static __device__ __forceinline__ void decided(const state_t& st, int32_t v, int32_t, int32_t, int lane,
                                                 const self_t& self, int32_t own_kvc, unsigned long long best,
                                                 int32_t label, tally_t&) {
    if (lane == 0 && moves<NARROW>(st, self, own_kvc, best))
      lpa_store<NARROW>(st.label + v, label);
  }
  /// The class's moves reach tot before the next class reads it: labels and tot pass from class to
  /// class inside the launch, fenced before the barriers.
  static __device__ __forceinline__ void class_done(const state_t& st, const int32_t* order, int32_t b0, int32_t b4,
                                                    tally_t& tally) {
    __threadfence();
    __syncthreads();  // the class is decided
    for (int32_t r = b0 + (int32_t)threadIdx.x; r < b4; r += LPA_BIG_BLOCK) {
      const int32_t v = order[r];
      louvain_apply(st, v, load_relaxed(st.label + v), tally.moved);
    }
    __threadfence();
  }
  template <bool NARROW>
  static __device__ __forceinline__ void flush(tally_t tally, counters_t* ctr) {
    if (NARROW) {
      const unsigned long long moved = wave_sum(tally.moved);
      if (lane_id() == 0 && moved)
        atomicAdd(&ctr->moves, moved);
    }
  }
};

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

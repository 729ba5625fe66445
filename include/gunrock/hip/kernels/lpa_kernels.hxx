/**
 * @file lpa_kernels.hxx
 * @brief Community detection (grx_lpa): semi-synchronous label propagation (Cordasco, Gargano 2010)
 * over the colour classes of grx_color, and the modularity of a labelling (grx_modularity).
 *
 * The sweep -- the schedule, the table of (label, count) and the kernels that decide a colour class
 * at once -- is class_sweep.hxx; this header is label propagation's decision, lpa_decision_t, and
 * the passes around the sweeps.  A decision is the most frequent label over the row's entries other
 * than self loops.  The vertex keeps its label when that is among the maxima and takes the maximum
 * of smallest fmix32(label) otherwise.  Counts are integers, so the answer does not depend on the
 * order of the inserts.
 *
 *   lpa_init_kernel            label[v] = v, dirty[v] = 1.
 *   lpa_publish_kernel         the sweep's hand-off: the change count and the entries read.
 *   lpa_canonical_kernel       label[v] = the smallest vertex id of its label (lpa_first_kernel), and
 *                              the communities counted.
 *   lpa_range_kernel, lpa_tot_kernel   modularity in integers: the range check and tot per label;
 *                              I and S are the unweighted score passes of class_sweep.hxx.
 *
 * Dirty flags, a byte per vertex: a vertex decides only while its flag is set and clears it; a
 * vertex that changes its label sets the flag of every other vertex in its row.  A vertex none of
 * whose neighbours changed since its last decision would decide the same.  Within a launch the
 * flags set belong to other classes and the flags cleared to this one: nothing is handed between
 * workgroups inside a launch.  The one-workgroup kernel does hand labels and flags from class to
 * class; there they are read and written with agent-scope relaxed accesses behind the workgroup's
 * barrier.
 *
 * The kernels are `inline`: capi_lpa.hip and capi_louvain.hip both include class_sweep.hxx.
 */
#pragma once

#include <gunrock/hip/kernels/class_sweep.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

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

/// Larger for the larger count, then for the smaller fmix32(label); 0 is below every entry's rank.
__device__ __forceinline__ unsigned long long lpa_rank(int32_t count, int32_t label) {
  return ((unsigned long long)(unsigned)count << 32) | (0xffffffffu - fmix32((unsigned)label));
}

/// Label propagation's decision (class_sweep.hxx says what each member is for).  The score of a
/// slot is lpa_rank: fmix32 is a bijection, so ONE slot holds the best score and its label is the
/// tie-break; v's own slot competes, and v moves when the best count is not its own label's.
struct lpa_decision_t {
  using state_t = lpa_state_t;
  using counters_t = lpa_counters_t;
  struct self_t {
    int32_t cur;
  };
  struct tally_t {
    unsigned long long read, changed;
  };
  using tie_t = int32_t;
  static constexpr tie_t no_tie = -1;
  static constexpr bool own_competes = true;
  static constexpr void (*apply_kernel)(state_t, const int32_t*, int32_t, counters_t*) = nullptr;

  template <bool NARROW>
  static __device__ __forceinline__ bool wants(const state_t& st, int32_t v) {
    return !st.dirty || lpa_load<NARROW>(st.dirty + v);
  }
  static __device__ __forceinline__ int32_t weight(const state_t&, int64_t) { return 1; }
  template <bool NARROW>
  static __device__ __forceinline__ self_t self(const state_t& st, int32_t v) {
    return {lpa_load<NARROW>(st.label + v)};
  }
  template <bool NARROW>
  static __device__ __forceinline__ void consider(const state_t&, const self_t&, int32_t label, int32_t count,
                                                  unsigned long long& score, tie_t& tie) {
    const unsigned long long r = lpa_rank(count, label);
    if (r > score) {
      score = r;
      tie = label;
    }
  }
  static __device__ __forceinline__ tie_t first_tie(tie_t a, tie_t b) { return max(a, b); }
  static __device__ __forceinline__ void offer(tie_t* word, tie_t tie) { *word = tie; }  // one slot has the rank
  static __device__ __forceinline__ int32_t label_of(tie_t tie) { return tie; }
  /// v moves when the best count is not its own label's.  The entries read, the flag cleared, and
  /// when v moved the label written, the change counted and its row marked.
  template <bool NARROW, int WIDTH>
  static __device__ __forceinline__ void decided(const state_t& st, int32_t v, int32_t lo, int32_t hi, int lane,
                                                 const self_t&, int32_t own, unsigned long long best, int32_t label,
                                                 tally_t& tally) {
    const bool moved = best != 0 && (int32_t)(best >> 32) != own;
    if (lane == 0) {
      tally.read += (unsigned long long)(hi - lo);
      if (st.dirty)
        lpa_store<NARROW>(st.dirty + v, (unsigned char)0);
      if (moved) {
        lpa_store<NARROW>(st.label + v, label);
        ++tally.changed;
        if (st.dirty)
          tally.read += (unsigned long long)(hi - lo);
      }
    }
    if (moved && st.dirty)
      for (int32_t e = lo + lane; e < hi; e += WIDTH) {
        const int32_t u = st.aj[e];
        if (u != v)
          lpa_store<NARROW>(st.dirty + u, (unsigned char)1);
      }
  }
  static __device__ __forceinline__ void class_done(const state_t&, const int32_t*, int32_t, int32_t, tally_t&) {}
  template <bool NARROW>
  static __device__ __forceinline__ void flush(tally_t tally, counters_t* ctr) {
    const unsigned long long read = wave_sum(tally.read), changed = wave_sum(tally.changed);
    if (lane_id() == 0) {
      if (read)
        atomicAdd(&ctr->read, read);
      if (changed)
        atomicAdd(&ctr->changes, changed);
    }
  }
};

inline __global__ void __launch_bounds__(LPA_BLOCK) lpa_init_kernel(int32_t* label, unsigned char* dirty, int32_t n) {
  for (int64_t v = blockIdx.x * (int64_t)LPA_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * LPA_BLOCK) {
    label[v] = (int32_t)v;
    if (dirty)
      dirty[v] = 1;
  }
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

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

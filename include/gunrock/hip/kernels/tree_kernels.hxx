/**
 * @file tree_kernels.hxx
 * @brief Shortest-path trees from finished labels (grx_bfs_predecessors, grx_sssp_predecessors): one
 * pass over the entries finds for every vertex the smallest neighbour its label follows from and
 * counts the entries that contradict the labels; pointer doubling turns the tree into hop counts.
 *
 * An entry (u, v, w) with label[u] reached is tested by tree_rule_t: BFS in 64-bit integers,
 * SSSP with ONE float32 add, the add every relaxation of grx_sssp performs, so at a fixed point the
 * equality holds bit for bit.  Two forms of the pass give the same answer:
 *
 *   pull   over in-rows.  A 16-lane group tests the entries of one vertex v (the sweep of
 *          group_rows.hxx), each lane keeps its smallest qualifying u, and the 16 minima meet in the
 *          butterfly; one lane stores pred[v] already mapped to source / -1 / -2.  No atomics.
 *   push   over out-rows.  pred starts at TREE_NONE; the group reads the owner's label once, skips the
 *          row of an unreached owner (it neither qualifies nor violates) and lowers pred[v] of every
 *          qualifying entry by a pre-tested atomicMin; tree_finalise_kernel maps what is left.
 *
 * Rows of more than `segment` entries are cut into items by group_plan_kernel and a group tests one
 * item; in the pull form the items of a row meet by pre-tested atomicMin on pred[v],
 * which tree_rows_kernel left at TREE_NONE, and tree_fixup_kernel maps the long rows.  A minimum, an
 * integer sum and a plain store do not depend on the order: a call repeats itself bit for bit.
 *
 * Counts (reached labels, orphans, violating entries) are summed per wavefront, then one 64-bit
 * atomic add per wavefront and non-zero count; the three words sit on lines of their own.
 *
 * Hops: pair[v] = {ancestor, steps to it}, 8 bytes, in two buffers that take turns.  Every end of a
 * chain points at itself with 0 steps (the source, an orphan, an unreached vertex), so a round is
 * pair'[v] = {pair[a].ancestor, steps + pair[a].steps} with a = pair[v].ancestor, and changes v
 * exactly while a is not an end.  After ceil(log2(L)) changing rounds every vertex names the end of
 * its chain, L the longest chain; a vertex whose end is not the source is dead: hops -1.  A round
 * reads one buffer and writes the other: in place it would read pairs another lane is replacing.
 * A round past the last changing one copies its input, so the host enqueues TREE_ROUNDS_AHEAD rounds
 * per hand-off, each with a word of its own that says whether it moved a pair, and stops after the
 * batch that holds the first round that moved none.
 */
#pragma once

#include <cfloat>

#include <gunrock/hip/kernels/group_rows.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int32_t TREE_NONE = INT32_MAX;  // pred[v] while no qualifying entry was seen
constexpr int32_t TREE_UNREACHED = -1, TREE_ORPHAN = -2;

/// The call's device words, 128 bytes apart.
enum { TREE_N_REACHED = 0, TREE_N_ORPHANS = 16, TREE_N_VIOLATIONS = 32, TREE_CHANGED = 48, TREE_WORDS = 64 };
constexpr int TREE_ROUNDS_AHEAD = 4;  // doubling rounds enqueued per hand-off, a word at TREE_CHANGED each
enum { TM_CHANGED = 0 };              // first mirror word of that hand-off: TREE_ROUNDS_AHEAD of them

/// When does an entry (u, v, w) with label[u] = lu reached and label[v] = lv qualify or violate?
template <typename label_t>
struct tree_rule_t;
template <>
struct tree_rule_t<int32_t> {
  static constexpr bool weighted = false;
  static constexpr int32_t unreached = INT32_MAX;
  __device__ static __forceinline__ void test(int32_t lu, float, int32_t lv, bool& qualifies, bool& violates) {
    const int64_t c = (int64_t)lu + 1;
    qualifies = c == (int64_t)lv;
    violates = c < (int64_t)lv;
  }
};
template <>
struct tree_rule_t<float> {
  static constexpr bool weighted = true;
  static constexpr float unreached = FLT_MAX;
  __device__ static __forceinline__ void test(float lu, float w, float lv, bool& qualifies, bool& violates) {
    const float c = __fadd_rn(lu, w);  // a NaN makes every comparison false
    qualifies = c == lv && lu < lv;
    violates = c < lv;
  }
};

/// Ends a counting kernel; every lane of the wavefront calls it.
__device__ __forceinline__ void tree_flush(unsigned long long count, unsigned long long* word) {
  count = wave_sum(count);
  if (lane_id() == 0 && count)
    atomicAdd(word, count);
}

/// The delivered pred[v] from the smallest qualifying u (TREE_NONE: none).
__device__ __forceinline__ int32_t tree_deliver(int32_t v, int32_t source, bool reached, int32_t best,
                                                unsigned long long& orphans) {
  if (v == source)
    return source;
  if (!reached)
    return TREE_UNREACHED;
  if (best == TREE_NONE) {
    ++orphans;
    return TREE_ORPHAN;
  }
  return best;
}

/**
 * @brief Entries [lo, hi) of `owner`'s row by one 16-lane group.  PUSH: the row is an out-row, the
 * owner (label `mine`, reached) is u and pred[] of the far end is lowered.  Pull: the row is an in-row,
 * the owner is v and the group's smallest qualifying u lands in `best`, in all its lanes.  Every lane of
 * the wavefront calls it (an empty range does nothing).
 */
template <typename label_t, bool PUSH>
__device__ __forceinline__ void tree_group_walk(const csr_rows_t& rows, const label_t* labels, int32_t owner,
                                                label_t mine, int32_t lo, int32_t hi, int lane, int32_t* pred,
                                                int32_t& best, unsigned long long& violations) {
  using rule = tree_rule_t<label_t>;
  group_walk<rule::weighted>(
      rows, lo, hi, lane, [&](int32_t c) { return labels[c]; },
      [&](int32_t c, float w, label_t far) {
        bool qualifies = false, violates = false;
        if (PUSH) {
          rule::test(mine, w, far, qualifies, violates);
          if (qualifies && load_relaxed(&pred[c]) > owner)
            atomicMin(&pred[c], owner);
        } else if (far != rule::unreached) {
          rule::test(far, w, mine, qualifies, violates);
          if (qualifies)
            best = min(best, c);
        }
        violations += violates ? 1u : 0u;
      });
  if (!PUSH)
    best = group_butterfly(best, [](int32_t a, int32_t b) { return min(a, b); });
}

/// Push form, first: pred[v] = TREE_NONE.
template <int header_only = 0>
__global__ void __launch_bounds__(GROUP_BLOCK) tree_fill_kernel(int32_t* pred, int32_t n) {
  for (int64_t v = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * GROUP_BLOCK)
    pred[v] = TREE_NONE;
}

/**
 * @brief Every row of at most `segment` entries, a lane group each.  Pull: stores the delivered
 * pred[v] (TREE_NONE for a longer row, which tree_segment_kernel and tree_fixup_kernel finish) and
 * counts the reached labels of ALL rows and the orphans among the short ones.  Push: lowers pred[].
 * Both count the violating entries they test.
 */
template <typename label_t, bool PUSH>
__global__ void __launch_bounds__(GROUP_BLOCK)
    tree_rows_kernel(csr_rows_t rows, const label_t* labels, int32_t n, int32_t segment, int32_t source,
                     int32_t* pred, unsigned long long* counts) {
  using rule = tree_rule_t<label_t>;
  unsigned long long reached = 0, orphans = 0, violations = 0;
  group_sweep_rows(
      rows.ap, n, segment, [&](int64_t v) { return labels[v]; },
      [&](int64_t v, int32_t lo, int32_t hi, bool in_range, bool is_short, label_t mine, int lane) {
        const bool is_reached = in_range && mine != rule::unreached;
        // an out-row of an unreached owner neither qualifies nor violates; an in-row of one can violate
        const bool walk = is_short && (!PUSH || is_reached);
        int32_t best = TREE_NONE;
        tree_group_walk<label_t, PUSH>(rows, labels, (int32_t)v, mine, lo, walk ? hi : lo, lane, pred, best,
                                       violations);
        if (!PUSH && in_range && lane == 0) {
          reached += is_reached ? 1u : 0u;
          pred[v] = is_short ? tree_deliver((int32_t)v, source, is_reached, best, orphans) : TREE_NONE;
        }
      });
  if (!PUSH) {
    tree_flush(reached, &counts[TREE_N_REACHED]);
    tree_flush(orphans, &counts[TREE_N_ORPHANS]);
  }
  tree_flush(violations, &counts[TREE_N_VIOLATIONS]);
}

/// Every item of the long rows, a lane group each.  Pull: the items of a row meet in pred[v].
template <typename label_t, bool PUSH>
__global__ void __launch_bounds__(GROUP_BLOCK)
    tree_segment_kernel(csr_rows_t rows, const label_t* labels, group_plan_t plan, int32_t segment, int32_t* pred,
                        unsigned long long* counts) {
  using rule = tree_rule_t<label_t>;
  unsigned long long violations = 0;
  group_sweep_items(rows.ap, plan, segment, [&](int64_t, int32_t v, int32_t lo, int32_t hi, bool live, int lane) {
    const label_t mine = live ? labels[v] : rule::unreached;
    const bool walk = !PUSH || mine != rule::unreached;  // as in tree_rows_kernel
    int32_t best = TREE_NONE;
    tree_group_walk<label_t, PUSH>(rows, labels, v, mine, lo, walk ? hi : lo, lane, pred, best, violations);
    if (!PUSH && live && lane == 0 && best != TREE_NONE && load_relaxed(&pred[v]) > best)
      atomicMin(&pred[v], best);
  });
  tree_flush(violations, &counts[TREE_N_VIOLATIONS]);
}

/// Pull form, last: the long rows' pred[v], a thread each, from what their items left.
template <typename label_t>
__global__ void __launch_bounds__(GROUP_BLOCK)
    tree_fixup_kernel(const label_t* labels, group_plan_t plan, int32_t source, int32_t* pred,
                      unsigned long long* counts) {
  const int32_t n_long = min(plan.counts[0], plan.most_rows);
  unsigned long long orphans = 0;
  for (int64_t j = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; j < n_long; j += (int64_t)gridDim.x * GROUP_BLOCK) {
    const int32_t v = plan.rows[j].x;
    pred[v] = tree_deliver(v, source, labels[v] != tree_rule_t<label_t>::unreached, pred[v], orphans);
  }
  tree_flush(orphans, &counts[TREE_N_ORPHANS]);
}

/// Push form, last: every pred[v], a thread each; counts the reached labels and the orphans.
template <typename label_t>
__global__ void __launch_bounds__(GROUP_BLOCK)
    tree_finalise_kernel(const label_t* labels, int32_t n, int32_t source, int32_t* pred, unsigned long long* counts) {
  unsigned long long reached = 0, orphans = 0;
  for (int64_t v = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * GROUP_BLOCK) {
    const bool is_reached = labels[v] != tree_rule_t<label_t>::unreached;
    reached += is_reached ? 1u : 0u;
    pred[v] = tree_deliver((int32_t)v, source, is_reached, pred[v], orphans);
  }
  tree_flush(reached, &counts[TREE_N_REACHED]);
  tree_flush(orphans, &counts[TREE_N_ORPHANS]);
}

/// Hops begin: a vertex with a predecessor other than itself is one step from it; all others end a chain.
template <int header_only = 0>
__global__ void __launch_bounds__(GROUP_BLOCK) tree_hops_begin_kernel(const int32_t* pred, int32_t n, int2* pair) {
  for (int64_t v = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * GROUP_BLOCK) {
    const int32_t p = pred[v];
    pair[v] = p >= 0 && p != (int32_t)v ? make_int2(p, 1) : make_int2((int32_t)v, 0);
  }
}

/// One doubling round from `old` into `now`; leaves 1 in *changed when a pair moved.
template <int header_only = 0>
__global__ void __launch_bounds__(GROUP_BLOCK)
    tree_hops_round_kernel(const int2* old, int2* now, int32_t n, unsigned long long* changed) {
  bool moved = false;
  for (int64_t v = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * GROUP_BLOCK) {
    int2 p = old[v];
    const int2 q = old[p.x];
    if (q.x != p.x) {  // the ancestor is not the end of its chain
      p = make_int2(q.x, p.y + q.y);
      moved = true;
    }
    now[v] = p;
  }
  if (__any(moved) && lane_id() == 0)
    store_relaxed(changed, 1ull);
}

/// Ends a batch of doubling rounds: one thread hands their words to the host and clears them.
template <int header_only = 0>
__global__ void tree_hops_publish_kernel(unsigned long long* changed, unsigned long long* mirror, int sequence_slot,
                                         unsigned long long sequence) {
  if (threadIdx.x != 0)
    return;
  for (int j = 0; j < TREE_ROUNDS_AHEAD; ++j)
    mirror[TM_CHANGED + j] = __hip_atomic_exchange(&changed[j], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  stamp_handoff(mirror, sequence_slot, sequence);
}

/// Hops end: the steps of a vertex whose chain ends at the source, -1 for every other.
template <int header_only = 0>
__global__ void __launch_bounds__(GROUP_BLOCK)
    tree_hops_end_kernel(const int2* pair, int32_t n, int32_t source, int32_t* hops) {
  for (int64_t v = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * GROUP_BLOCK) {
    const int2 p = pair[v];
    hops[v] = p.x == source ? p.y : -1;
  }
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

/**
 * @file softmax_kernels.hxx
 * @brief The softmax of per-entry scores over the entries that share a row, or a column
 * (grx_edge_softmax), and its derivative (grx_edge_softmax_backward): streams of 4-byte values with no
 * gather -- the offsets and the per-entry arrays are all that is read; no column id, no value of the CSR.
 *
 * A group is a row of the offsets handed in: the CSR's, or the in-rows', whose entry j stands for entry
 * at_of[j] of the CSR (INDIRECT: the in-edges' entry ids).  A 16-lane group takes one group of at most
 * `segment` entries by the sweep of group_rows.hxx and passes over it three times, each lane over the
 * same entries every time: the maximum (a butterfly), the sum of exp(s - max) in grx_spmv's order (lane
 * l adds entries l, l + 16, ... from 0.0f, then the butterfly), and the quotients, whose numerators are
 * computed again rather than kept.  A longer group is cut into the plan's items {row, k}, a lane group
 * each, and the same three steps are kernels: the items' maxima meet in one word per long row, the
 * items' sums go to partial[] and one thread per long row adds them in segment order, an item sweep
 * writes.  The word, the partials and the total of a long row sit at the index of its first item, which
 * item i of segment k knows as i - k.
 *
 * The maximum is taken over order-preserving keys (softmax_key): unsigned integers that order like the
 * floats, every NaN above +inf.  A maximum of integers does not depend on order, so the long rows may
 * use atomicMax; and a NaN anywhere in a group makes its maximum NaN, also beside -inf.  A group whose
 * maximum is -inf is fully masked and gets 0.0f.  No float atomic, no kernel that waits on another
 * workgroup; the order of every sum depends on the group's length and `segment` alone.
 */
#pragma once

#include <gunrock/hip/kernels/group_rows.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

/// What the kernels of one call share: offsets, the entries' positions (INDIRECT) and the segment.
struct softmax_groups_t {
  const int32_t* ap;
  const int32_t* at_of;
  int32_t n, segment;
};

constexpr unsigned SOFTMAX_KEY_NAN = 0xffffffffu;
constexpr unsigned SOFTMAX_KEY_MASKED = 0x007fffffu;  // the key of -inf; every key is above 0

/// a < b as floats <=> key(a) < key(b) as unsigned; -0 below +0; every NaN has the largest key.
__device__ __forceinline__ unsigned softmax_key(float x) {
  const unsigned u = __float_as_uint(x);
  if (x != x)
    return SOFTMAX_KEY_NAN;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float softmax_unkey(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

/// The largest key of entries [lo, hi), valid in all 16 lanes; 0 for an empty range.
template <bool INDIRECT>
__device__ __forceinline__ unsigned softmax_group_max(const softmax_groups_t& g, const float* s, int32_t lo,
                                                      int32_t hi, int lane) {
  unsigned key = 0;
  group_walk_entries<INDIRECT, false>(s, nullptr, g.at_of, lo, hi, lane,
                                      [&](uint32_t, float x, float) { key = max(key, softmax_key(x)); });
  return group_butterfly(key, [](unsigned a, unsigned b) { return max(a, b); });
}

/// p[e] = expf(s[e] - m): one rounded subtraction and the precise exponential.
__device__ __forceinline__ float softmax_term(float s, float m) { return expf(__fsub_rn(s, m)); }

/// The sum of p over entries [lo, hi) in grx_spmv's order, valid in all 16 lanes.
template <bool INDIRECT>
__device__ __forceinline__ float softmax_group_sum(const softmax_groups_t& g, const float* s, float m, int32_t lo,
                                                   int32_t hi, int lane) {
  float acc = 0.0f;
  group_walk_entries<INDIRECT, false>(s, nullptr, g.at_of, lo, hi, lane,
                                      [&](uint32_t, float x, float) { acc = __fadd_rn(acc, softmax_term(x, m)); });
  return group_butterfly(acc, [](float a, float b) { return __fadd_rn(a, b); });
}

/// out[e] = p[e] / total for entries [lo, hi); 0.0f where the group's maximum is -inf.
template <bool INDIRECT>
__device__ __forceinline__ void softmax_group_write(const softmax_groups_t& g, const float* s, unsigned max_key,
                                                    float total, int32_t lo, int32_t hi, int lane, float* out) {
  const float m = softmax_unkey(max_key);
  const bool masked = max_key == SOFTMAX_KEY_MASKED;
  group_walk_entries<INDIRECT, false>(s, nullptr, g.at_of, lo, hi, lane, [&](uint32_t at, float x, float) {
    out[at] = masked ? 0.0f : __fdiv_rn(softmax_term(x, m), total);
  });
}

/// D = the sum of fma(a[e], t[e], acc) over entries [lo, hi) in the same order, valid in all 16 lanes.
template <bool INDIRECT>
__device__ __forceinline__ float softmax_group_dot(const softmax_groups_t& g, const float* a, const float* t,
                                                   int32_t lo, int32_t hi, int lane) {
  float acc = 0.0f;
  group_walk_entries<INDIRECT, true>(a, t, g.at_of, lo, hi, lane,
                                     [&](uint32_t, float x, float y) { acc = __fmaf_rn(x, y, acc); });
  return group_butterfly(acc, [](float x, float y) { return __fadd_rn(x, y); });
}

/// out[e] = a[e] * (t[e] - D) for entries [lo, hi).
template <bool INDIRECT>
__device__ __forceinline__ void softmax_group_scale(const softmax_groups_t& g, const float* a, const float* t,
                                                    float dot, int32_t lo, int32_t hi, int lane, float* out) {
  group_walk_entries<INDIRECT, true>(a, t, g.at_of, lo, hi, lane, [&](uint32_t at, float x, float y) {
    out[at] = __fmul_rn(x, __fsub_rn(y, dot));
  });
}

/// Item i of a long row: its segment k and the index its row's word, partials' total and maximum sit at.
__device__ __forceinline__ int64_t softmax_row_slot(const group_plan_t& plan, int64_t i, bool live) {
  return live ? i - plan.items[i].y : 0;
}

/// Forward, every group of at most `segment` entries, a lane group each.
template <bool INDIRECT>
__global__ void __launch_bounds__(GROUP_BLOCK) softmax_rows_kernel(softmax_groups_t g, const float* s, float* out) {
  group_sweep_rows(
      g.ap, g.n, g.segment, [](int64_t) { return 0; },
      [&](int64_t, int32_t lo, int32_t hi, bool, bool is_short, int, int lane) {
        if (!is_short)  // the item kernels write the longer groups
          hi = lo;
        const unsigned max_key = softmax_group_max<INDIRECT>(g, s, lo, hi, lane);
        const float total = softmax_group_sum<INDIRECT>(g, s, softmax_unkey(max_key), lo, hi, lane);
        softmax_group_write<INDIRECT>(g, s, max_key, total, lo, hi, lane, out);
      });
}

/// Forward, long groups, first of four: max_keys[slot] = the largest key of the row; zero before.
template <bool INDIRECT>
__global__ void __launch_bounds__(GROUP_BLOCK)
    softmax_item_max_kernel(softmax_groups_t g, group_plan_t plan, const float* s, unsigned* max_keys) {
  group_sweep_items(g.ap, plan, g.segment, [&](int64_t i, int32_t, int32_t lo, int32_t hi, bool live, int lane) {
    const unsigned key = softmax_group_max<INDIRECT>(g, s, lo, hi, lane);
    if (live && lane == 0)
      atomicMax(&max_keys[softmax_row_slot(plan, i, live)], key);
  });
}

/// Forward, long groups, second: partial[i] = the sum of p over item i.
template <bool INDIRECT>
__global__ void __launch_bounds__(GROUP_BLOCK)
    softmax_item_sum_kernel(softmax_groups_t g, group_plan_t plan, const float* s, const unsigned* max_keys,
                            float* partial) {
  group_sweep_items(g.ap, plan, g.segment, [&](int64_t i, int32_t, int32_t lo, int32_t hi, bool live, int lane) {
    const float m = softmax_unkey(load_relaxed(&max_keys[softmax_row_slot(plan, i, live)]));
    const float acc = softmax_group_sum<INDIRECT>(g, s, m, lo, hi, lane);
    if (live && lane == 0)
      partial[i] = acc;
  });
}

/// Both directions, long groups, third: total[slot] = the row's partials in segment order, a thread each.
template <int header_only = 0>
__global__ void __launch_bounds__(GROUP_BLOCK)
    softmax_combine_kernel(softmax_groups_t g, group_plan_t plan, const float* partial, float* total) {
  const int32_t n_long = min(plan.counts[0], plan.most_rows);
  for (int64_t j = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; j < n_long; j += (int64_t)gridDim.x * GROUP_BLOCK) {
    const int2 row = plan.rows[j];
    const int32_t segments = (g.ap[row.x + 1] - g.ap[row.x] + g.segment - 1) / g.segment;
    float acc = 0.0f;
    for (int32_t k = 0; k < segments; ++k)
      if (row.y + k < plan.most_items)
        acc = __fadd_rn(acc, partial[row.y + k]);
    if (row.y < plan.most_items)
      total[row.y] = acc;
  }
}

/// Forward, long groups, fourth: the quotients of item i.
template <bool INDIRECT>
__global__ void __launch_bounds__(GROUP_BLOCK)
    softmax_item_write_kernel(softmax_groups_t g, group_plan_t plan, const float* s, const unsigned* max_keys,
                              const float* total, float* out) {
  group_sweep_items(g.ap, plan, g.segment, [&](int64_t i, int32_t, int32_t lo, int32_t hi, bool live, int lane) {
    const int64_t slot = softmax_row_slot(plan, i, live);
    softmax_group_write<INDIRECT>(g, s, load_relaxed(&max_keys[slot]), total[slot], lo, hi, lane, out);
  });
}

/// Backward, every group of at most `segment` entries, a lane group each.
template <bool INDIRECT>
__global__ void __launch_bounds__(GROUP_BLOCK)
    softmax_backward_rows_kernel(softmax_groups_t g, const float* a, const float* t, float* out) {
  group_sweep_rows(
      g.ap, g.n, g.segment, [](int64_t) { return 0; },
      [&](int64_t, int32_t lo, int32_t hi, bool, bool is_short, int, int lane) {
        if (!is_short)
          hi = lo;
        const float dot = softmax_group_dot<INDIRECT>(g, a, t, lo, hi, lane);
        softmax_group_scale<INDIRECT>(g, a, t, dot, lo, hi, lane, out);
      });
}

/// Backward, long groups, first of three: partial[i] = D over item i.
template <bool INDIRECT>
__global__ void __launch_bounds__(GROUP_BLOCK)
    softmax_backward_item_sum_kernel(softmax_groups_t g, group_plan_t plan, const float* a, const float* t,
                                     float* partial) {
  group_sweep_items(g.ap, plan, g.segment, [&](int64_t i, int32_t, int32_t lo, int32_t hi, bool live, int lane) {
    const float acc = softmax_group_dot<INDIRECT>(g, a, t, lo, hi, lane);
    if (live && lane == 0)
      partial[i] = acc;
  });
}

/// Backward, long groups, third (behind softmax_combine_kernel): the results of item i.
template <bool INDIRECT>
__global__ void __launch_bounds__(GROUP_BLOCK)
    softmax_backward_item_write_kernel(softmax_groups_t g, group_plan_t plan, const float* a, const float* t,
                                       const float* total, float* out) {
  group_sweep_items(g.ap, plan, g.segment, [&](int64_t i, int32_t, int32_t lo, int32_t hi, bool live, int lane) {
    softmax_group_scale<INDIRECT>(g, a, t, total[softmax_row_slot(plan, i, live)], lo, hi, lane, out);
  });
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

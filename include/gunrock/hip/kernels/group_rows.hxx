/**
 * @file group_rows.hxx
 * @brief The lane-group pull sweep over weighted CSR rows that the SpMV family (spmv_kernels.hxx) and
 * the tree family (tree_kernels.hxx) share; what is gathered through a column id and what becomes of
 * an entry is the caller's.  The edge softmax (softmax_kernels.hxx) takes the sweep with a walk over
 * per-entry arrays alone (group_walk_entries).
 *
 * A 16-lane group takes one row: lane l walks entries l, l + 16, ... in order, GROUP_FLIGHT of them in
 * flight, and the 16 lanes meet in a butterfly.  A wavefront holds four groups, a workgroup sixteen;
 * R-MAT rows are about 16 entries, so a group reads one 64-byte segment of column ids per step.  A
 * row of more than `segment` entries is cut once per call (group_plan_kernel) into items {row, k} of
 * `segment` entries, a group each, and a kernel of the caller's finishes the long rows.  What a lane
 * meets in which order depends on the row's layout and `segment` alone, never on the grid, the CU
 * count or arrival order; where an item sits in the list varies from run to run (integer atomics).
 * Every lane of a wavefront reaches the body of every step of both sweeps, so a body may hold a
 * butterfly: a lane group without a row or item of its own walks an empty range.
 */
#pragma once

#include <gunrock/hip/kernels/row_walk.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int GROUP_BLOCK = 256;
constexpr int GROUP_LANES = 16;                          // lanes that share a row
constexpr int GROUP_ROWS = GROUP_BLOCK / GROUP_LANES;    // rows a workgroup walks side by side
constexpr int GROUP_SEGMENT = 512;                       // default: row entries one lane group walks
constexpr int GROUP_SEGMENT_MIN = 64;
constexpr int GROUP_FLIGHT = 4;                          // entries in flight per lane

/// Weighted rows: the CSR, or the attached in-edge arrays.
struct csr_rows_t {
  const int32_t* ap;
  const int32_t* aj;
  const float* ax;
};

/// The long rows of one csr_rows_t: rows[j] = {row, its first item}, items[i] = {row, segment}.
struct group_plan_t {
  int32_t* counts;  // [0] long rows, [1] items; zero before group_plan_kernel
  int2* rows;
  int2* items;
  int32_t most_rows, most_items;  // what the arrays hold (sized by the host from nnz)
};

/**
 * @brief Entries [lo, hi) by one lane group: per entry gather(c) through its column id, then
 * consume(c, w, gathered) -- per lane slot 0 to 3 within an iteration, iterations ascending.  w is 0
 * without WEIGHTED, which reads no weights.  lo and hi lie within ap[], so below 2^31; the walk counts
 * in unsigned 32 bits, where e + 48 and e + 64 near the end of a CSR that fills its offsets cannot wrap.
 */
template <bool WEIGHTED, typename gather_t, typename consume_t>
__device__ __forceinline__ void group_walk(const csr_rows_t& rows, int32_t lo, int32_t hi, int lane,
                                           gather_t&& gather, consume_t&& consume) {
  for (uint32_t e = (uint32_t)lo + lane, end = (uint32_t)hi; e < end; e += GROUP_LANES * GROUP_FLIGHT) {
    int32_t c[GROUP_FLIGHT];
    float w[GROUP_FLIGHT];
    decltype(gather(0)) far[GROUP_FLIGHT];
#pragma unroll
    for (int k = 0; k < GROUP_FLIGHT; ++k) {  // a slot past the end reads nothing
      c[k] = 0;
      w[k] = 0.0f;
      if (e + k * GROUP_LANES < end) {
        c[k] = rows.aj[e + k * GROUP_LANES];
        if (WEIGHTED)
          w[k] = rows.ax[e + k * GROUP_LANES];
      }
    }
#pragma unroll
    for (int k = 0; k < GROUP_FLIGHT; ++k) {
      far[k] = {};
      if (e + k * GROUP_LANES < end)
        far[k] = gather(c[k]);
    }
#pragma unroll
    for (int k = 0; k < GROUP_FLIGHT; ++k)
      if (e + k * GROUP_LANES < end)
        consume(c[k], w[k], far[k]);
  }
}

/**
 * @brief Entries [lo, hi) of per-entry arrays by one lane group, group_walk without its column ids:
 * consume(at, a, b) with a = first[at] and b = second[at] (0 without TWO, which reads no second array),
 * at = at_of[e] with INDIRECT (the entry's position in the arrays: the in-edges' entry ids) and e
 * otherwise.  The same lanes meet the same entries in the same order as in group_walk, GROUP_FLIGHT of
 * them in flight.
 */
template <bool INDIRECT, bool TWO, typename consume_t>
__device__ __forceinline__ void group_walk_entries(const float* first, const float* second, const int32_t* at_of,
                                                   int32_t lo, int32_t hi, int lane, consume_t&& consume) {
  for (uint32_t e = (uint32_t)lo + lane, end = (uint32_t)hi; e < end; e += GROUP_LANES * GROUP_FLIGHT) {
    uint32_t at[GROUP_FLIGHT];
    float a[GROUP_FLIGHT], b[GROUP_FLIGHT];
#pragma unroll
    for (int k = 0; k < GROUP_FLIGHT; ++k) {  // a slot past the end reads nothing
      at[k] = e + k * GROUP_LANES;
      if (INDIRECT && at[k] < end)
        at[k] = (uint32_t)at_of[at[k]];
    }
#pragma unroll
    for (int k = 0; k < GROUP_FLIGHT; ++k) {
      a[k] = b[k] = 0.0f;
      if (e + k * GROUP_LANES < end) {
        a[k] = first[at[k]];
        if (TWO)
          b[k] = second[at[k]];
      }
    }
#pragma unroll
    for (int k = 0; k < GROUP_FLIGHT; ++k)
      if (e + k * GROUP_LANES < end)
        consume(at[k], a[k], b[k]);
  }
}

/// op over the 16 values of a lane group in a fixed order, valid in all its lanes.
template <typename value_t, typename op_t>
__device__ __forceinline__ value_t group_butterfly(value_t value, op_t&& op) {
#pragma unroll
  for (int d = GROUP_LANES / 2; d > 0; d >>= 1)
    value = op(value, __shfl_xor(value, d, wave_size));
  return value;
}

/**
 * @brief Every row, a lane group each: body(v, lo, hi, in_range, is_short, value, lane) once per step.
 * in_range: v < n; is_short: in range and at most `segment` entries, the rows the body walks.  value =
 * fetch(v), or 0 for a sweep that needs none: it comes in with the next step's offsets behind this
 * step's entries.
 */
template <typename fetch_t, typename body_t>
__device__ __forceinline__ void group_sweep_rows(const int32_t* ap, int32_t n, int32_t segment, fetch_t&& fetch,
                                                 body_t&& body) {
  const int group = (int)threadIdx.x / GROUP_LANES, lane = (int)threadIdx.x % GROUP_LANES;
  const int64_t stride = (int64_t)gridDim.x * GROUP_ROWS;
  int32_t lo, hi, lo_next, hi_next;
  using value_t = decltype(fetch(int64_t{}));
  value_t value, value_next;
  const auto row = [&](int64_t v, int32_t& from, int32_t& to, value_t& its) {
    from = to = 0;
    its = value_t{};
    if (v < n) {
      from = ap[v];
      to = ap[v + 1];
      its = fetch(v);
    }
  };
  row((int64_t)blockIdx.x * GROUP_ROWS + group, lo, hi, value);
  for (int64_t v0 = (int64_t)blockIdx.x * GROUP_ROWS; v0 < n; v0 += stride) {
    const int64_t v = v0 + group;
    row(v + stride, lo_next, hi_next, value_next);
    body(v, lo, hi, v < n, v < n && hi - lo <= segment, value, lane);
    lo = lo_next;
    hi = hi_next;
    value = value_next;
  }
}

/// Every item of the long rows, a lane group each: body(i, v, lo, hi, live, lane) once per step; a
/// group past the last item is not live and has an empty range.  The body may empty a live one.
template <typename body_t>
__device__ __forceinline__ void group_sweep_items(const int32_t* ap, const group_plan_t& plan, int32_t segment,
                                                  body_t&& body) {
  const int group = (int)threadIdx.x / GROUP_LANES, lane = (int)threadIdx.x % GROUP_LANES;
  const int32_t n_items = min(plan.counts[1], plan.most_items);
  for (int64_t i0 = (int64_t)blockIdx.x * GROUP_ROWS; i0 < n_items; i0 += (int64_t)gridDim.x * GROUP_ROWS) {
    const int64_t i = i0 + group;
    int32_t lo = 0, hi = 0, v = 0;
    if (i < n_items) {
      const int2 item = plan.items[i];
      v = item.x;
      const int64_t from = (int64_t)ap[v] + (int64_t)item.y * segment;  // from + segment may pass 2^31
      lo = (int32_t)from;
      hi = (int32_t)min((int64_t)ap[v + 1], from + segment);
    }
    body(i, v, lo, hi, i < n_items, lane);
  }
}

/// Once per call and row set: the rows of more than `segment` entries and their items.
template <int header_only = 0>
__global__ void __launch_bounds__(GROUP_BLOCK)
    group_plan_kernel(csr_rows_t rows, int32_t n, int32_t segment, group_plan_t plan) {
  for (int64_t v = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * GROUP_BLOCK) {
    const int32_t d = rows.ap[v + 1] - rows.ap[v];
    if (d <= segment)
      continue;
    const int32_t segments = (d + segment - 1) / segment;
    const int32_t j = atomicAdd(&plan.counts[0], 1);
    const int32_t at = atomicAdd(&plan.counts[1], segments);
    if (j < plan.most_rows)  // sized from nnz, so both hold; they guard the stores all the same
      plan.rows[j] = make_int2((int32_t)v, at);
    for (int32_t k = 0; k < segments; ++k)
      if (at + k < plan.most_items)
        plan.items[at + k] = make_int2((int32_t)v, k);
  }
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

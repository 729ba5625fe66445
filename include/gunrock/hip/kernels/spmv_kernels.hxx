/**
 * @file spmv_kernels.hxx
 * @brief Sparse matrix-vector products whose every row sum has a fixed order (grx_spmv), and the
 * HITS iteration built from two of them (grx_hits).
 *
 * A 16-lane group sums one row by the sweep of group_rows.hxx: lane l adds entries l, l + 16, ... in
 * order, one fused multiply-add each, and the 16 sums meet in the butterfly.  A lane group sums one
 * item of a long row the same way into partial[] and one thread per long row adds its partials in
 * segment order (spmv_combine_kernel).  The order of a sum depends on the row's layout and `segment`
 * alone: never on the grid, the CU count or arrival order.
 *
 * The operand may carry a scale: with SCALED the value read for column c is x[c] * r, r the rounded
 * reciprocal of a maximum an EARLIER kernel left in a device word (0 when that maximum is 0).  With
 * TRACK the kernel leaves the largest |sum| it wrote in such a word: per wavefront one butterfly and
 * at most one atomicMax on the bits of |value| -- floats without a sign order like unsigned integers,
 * NaN above all of them, and a maximum does not depend on the order.
 *
 * HITS keeps the unnormalised products y (authorities) and z[2] (hubs, two that take turns) and three
 * such words; the vectors of the definition are a_t = y * r(a_max), h_t = z[t & 1] * r(h_max[t & 1]).
 * Iteration t, in launch order:
 *
 *   gather / segment / combine   y    = in-rows  times (z[~t & 1] * r(h_max[~t & 1])), max into a_max
 *   gather / segment / combine   z[t] = out-rows times (y * r(a_max)),                max into h_max[t & 1]
 *   hits_residual_kernel         max |h_t - h_{t-1}| into diff (left out while nobody reads it)
 *   hits_step_kernel             one thread: iterations, residual, clears diff, a_max (kept in a_last)
 *                                and h_max[~t & 1] for iteration t + 1, and stamps the hand-off when
 *                                the host waits for it
 *
 * so normalising costs no pass of its own: the scale is applied where the value is gathered.  A word
 * is always read by a later kernel than the one that wrote it.  No float atomic, no kernel that waits
 * on another workgroup.
 */
#pragma once

#include <gunrock/hip/kernels/group_rows.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

/// Device words of a grx_hits call.
struct hits_ctl_t {
  unsigned a_max;      // bits of max |y| of the running iteration
  unsigned a_last;     // ... of the last finished one
  unsigned h_max[2];   // bits of max |z[i]|
  unsigned diff;       // bits of max |h_t - h_{t-1}|
  int32_t iterations;
  float residual;
  unsigned long long reached;
};
enum { HM_DIFF = 0, HM_WORDS };

__device__ __forceinline__ unsigned spmv_magnitude(float x) { return __float_as_uint(fabsf(x)); }

/// r with value * r = value / max: the rounded reciprocal, 0 when the maximum is 0.
__device__ __forceinline__ float spmv_reciprocal(const unsigned* max_bits) {
  const float m = __uint_as_float(load_relaxed(max_bits));
  return m == 0.0f ? 0.0f : __fdiv_rn(1.0f, m);
}

/// The sum over entries [lo, hi) as the header says; valid in all 16 lanes of the group.  Every lane of
/// the wavefront calls it (an empty range gives 0).
template <bool SCALED>
__device__ __forceinline__ float spmv_group_sum(const csr_rows_t& rows, const float* x, float r, int32_t lo,
                                                int32_t hi, int lane) {
  float acc = 0.0f;
  group_walk<true>(
      rows, lo, hi, lane, [&](int32_t c) { return x[c]; },
      [&](int32_t, float w, float v) { acc = __fmaf_rn(SCALED ? __fmul_rn(v, r) : v, w, acc); });
  return group_butterfly(acc, [](float a, float b) { return __fadd_rn(a, b); });
}

/// Ends a TRACK kernel: the wavefront's largest magnitude, at most one atomic.
__device__ __forceinline__ void spmv_flush_max(unsigned worst, unsigned* max_bits) {
  worst = wave_max(worst);
  if (lane_id() == 0 && worst)
    atomicMax(max_bits, worst);
}

/// y[v] for every row of at most `segment` entries, a lane group each.
template <bool SCALED, bool TRACK>
__global__ void __launch_bounds__(GROUP_BLOCK)
    spmv_gather_kernel(csr_rows_t rows, const float* x, const unsigned* scale_bits, int32_t n, int32_t segment,
                       float* y, unsigned* max_bits) {
  const float r = SCALED ? spmv_reciprocal(scale_bits) : 1.0f;
  unsigned worst = 0;
  group_sweep_rows(
      rows.ap, n, segment, [](int64_t) { return 0; },
      [&](int64_t v, int32_t lo, int32_t hi, bool, bool is_short, int, int lane) {
        const float acc = spmv_group_sum<SCALED>(rows, x, r, lo, is_short ? hi : lo, lane);
        if (is_short && lane == 0) {  // spmv_combine_kernel writes the longer rows
          y[v] = acc;
          if (TRACK)
            worst = max(worst, spmv_magnitude(acc));
        }
      });
  if (TRACK)
    spmv_flush_max(worst, max_bits);
}

/// partial[i] = the sum over item i of the long rows, a lane group each.
template <bool SCALED>
__global__ void __launch_bounds__(GROUP_BLOCK)
    spmv_segment_kernel(csr_rows_t rows, const float* x, const unsigned* scale_bits, group_plan_t plan,
                        int32_t segment, float* partial) {
  const float r = SCALED ? spmv_reciprocal(scale_bits) : 1.0f;
  group_sweep_items(rows.ap, plan, segment, [&](int64_t i, int32_t, int32_t lo, int32_t hi, bool live, int lane) {
    const float acc = spmv_group_sum<SCALED>(rows, x, r, lo, hi, lane);
    if (live && lane == 0)
      partial[i] = acc;
  });
}

/// y[v] of the long rows, a thread each: the partial sums in segment order.
template <bool TRACK>
__global__ void __launch_bounds__(GROUP_BLOCK)
    spmv_combine_kernel(csr_rows_t rows, group_plan_t plan, int32_t segment, const float* partial, float* y,
                        unsigned* max_bits) {
  const int32_t n_long = min(plan.counts[0], plan.most_rows);
  unsigned worst = 0;
  for (int64_t j = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; j < n_long; j += (int64_t)gridDim.x * GROUP_BLOCK) {
    const int2 row = plan.rows[j];
    const int32_t segments = (rows.ap[row.x + 1] - rows.ap[row.x] + segment - 1) / segment;
    float acc = 0.0f;
    for (int32_t k = 0; k < segments; ++k)
      if (row.y + k < plan.most_items)
        acc = __fadd_rn(acc, partial[row.y + k]);
    y[row.x] = acc;
    if (TRACK)
      worst = max(worst, spmv_magnitude(acc));
  }
  if (TRACK)
    spmv_flush_max(worst, max_bits);
}

/// A call begins: h_0 = 1 in z[0] with h_max[0] = 1; everything else is 0.  z[0] has n entries.
template <int header_only = 0>
__global__ void __launch_bounds__(GROUP_BLOCK) hits_begin_kernel(float* z0, int32_t n, hits_ctl_t* ctl) {
  for (int64_t v = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * GROUP_BLOCK)
    z0[v] = 1.0f;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctl->a_max = ctl->a_last = ctl->h_max[1] = ctl->diff = 0;
    ctl->h_max[0] = __float_as_uint(1.0f);
    ctl->iterations = 0;
    ctl->residual = 0.0f;
    ctl->reached = 0;
  }
}

/// max_v |h_t[v] - h_{t-1}[v]| into ctl->diff; `now` = t & 1.
template <int header_only = 0>
__global__ void __launch_bounds__(GROUP_BLOCK)
    hits_residual_kernel(const float* z0, const float* z1, int now, int32_t n, hits_ctl_t* ctl) {
  const float* z_now = now ? z1 : z0;
  const float* z_old = now ? z0 : z1;
  const float r_now = spmv_reciprocal(&ctl->h_max[now]), r_old = spmv_reciprocal(&ctl->h_max[now ^ 1]);
  unsigned worst = 0;
  for (int64_t v = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * GROUP_BLOCK)
    worst = max(worst, spmv_magnitude(__fsub_rn(__fmul_rn(z_now[v], r_now), __fmul_rn(z_old[v], r_old))));
  spmv_flush_max(worst, &ctl->diff);
}

/// Ends iteration t: one thread.  With a mirror the host waits for the stamp and reads the residual.
template <int header_only = 0>
__global__ void hits_step_kernel(hits_ctl_t* ctl, int32_t t, int measured, unsigned long long* mirror,
                                 int sequence_slot, unsigned long long sequence) {
  if (threadIdx.x != 0)
    return;
  // the words were changed by atomics: read and cleared past the caches
  const unsigned diff = __hip_atomic_exchange(&ctl->diff, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  ctl->a_last = __hip_atomic_exchange(&ctl->a_max, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  store_relaxed(&ctl->h_max[~t & 1], 0u);
  ctl->iterations = t;
  if (measured)
    ctl->residual = __uint_as_float(diff);
  if (mirror) {
    mirror[HM_DIFF] = diff;
    stamp_handoff(mirror, sequence_slot, sequence);
  }
}

/// Delivery: hub = z * r(h_max), authority = y * r(a_last), either may be NULL; counts the vertices
/// with a value > 0 in one of them.
template <int header_only = 0>
__global__ void __launch_bounds__(GROUP_BLOCK)
    hits_deliver_kernel(const float* z, const float* y, int now, int32_t n, float* hub, float* authority,
                        hits_ctl_t* ctl) {
  const float r_h = spmv_reciprocal(&ctl->h_max[now]), r_a = spmv_reciprocal(&ctl->a_last);
  unsigned count = 0;
  const int64_t stride = (int64_t)gridDim.x * GROUP_BLOCK;
  const int64_t span = ((int64_t)n + wave_size - 1) / wave_size * wave_size;  // whole wavefronts reach the ballot
  for (int64_t v = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; v < span; v += stride) {
    float h = 0.0f, a = 0.0f;
    if (v < n) {
      h = __fmul_rn(z[v], r_h);
      a = __fmul_rn(y[v], r_a);
      if (hub)
        hub[v] = h;
      if (authority)
        authority[v] = a;
    }
    count += (unsigned)__popcll(__ballot(h > 0.0f || a > 0.0f));
  }
  if (lane_id() == 0 && count)
    atomicAdd(&ctl->reached, (unsigned long long)count);
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

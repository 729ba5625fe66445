/**
 * @file near_far.hxx
 * @brief Near / far split of a pending set by an ADAPTIVE distance threshold (SSSP, DESIGN.md
 * section 5): the arithmetic shared by the device chooser (compact_kernels.hxx) and the host.
 *
 * Pending vertices add their out-degree to a histogram keyed by a monotone code of their distance
 * (the top 12 of the 16 bound bits: 8 bins per octave of a positive float).  The threshold is the
 * smallest code at which the cumulative work reaches a share `frac` of the total: everything at or
 * below it is expanded now, the rest stays pending while its labels keep falling.
 *
 * No HIP in here: the file compiles as plain C++ (tests/cpp/near_far_tests.cpp).
 */
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GRX_NEAR_HD __host__ __device__
#else
#define GRX_NEAR_HD
#endif

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int NEAR_SHIFT = 4;                     // code = bound16 >> 4
constexpr int NEAR_BINS = 1 << (16 - NEAR_SHIFT);  // 4096
constexpr unsigned NEAR_ALL = 0xffffu;            // threshold "every pending vertex" (above every code)

/// Monotone code of a distance from its 2-byte upper bound (sssp_problem_t::bound16).
GRX_NEAR_HD inline unsigned near_code(unsigned bound16) { return (bound16 & 0xffffu) >> NEAR_SHIFT; }

/// Cumulative work the near set must reach: the share `frac` of `total`, at least one edge.
GRX_NEAR_HD inline unsigned long long near_target(unsigned long long total, double frac) {
  if (!(frac > 0.0))
    frac = 0.0;
  if (frac >= 1.0)
    return total ? total : 1ull;
  const unsigned long long t = (unsigned long long)(frac * (double)total);
  return t ? t : 1ull;
}

/// The first of `count` consecutive bins at which `before` + the bins' running sum reaches `target`
/// (`before`: the work of all bins in front of them), or -1 when these bins do not reach it.
template <typename bin_t>
GRX_NEAR_HD inline int near_find(const bin_t* bins, int count, unsigned long long before,
                                 unsigned long long target) {
  if (before >= target)
    return -1;  // an earlier bin already did
  for (int i = 0; i < count; ++i) {
    before += (unsigned long long)bins[i];
    if (before >= target)
      return i;
  }
  return -1;
}

/// The whole choice, serially: NEAR_ALL when the pending work is nothing or below `min_total` (the
/// round then takes everything), else the smallest code whose cumulative work reaches the target.
template <typename bin_t>
GRX_NEAR_HD inline unsigned near_threshold(const bin_t* bins, int n_bins, unsigned long long min_total,
                                           double frac, unsigned long long* total_out = nullptr) {
  unsigned long long total = 0;
  for (int i = 0; i < n_bins; ++i)
    total += (unsigned long long)bins[i];
  if (total_out)
    *total_out = total;
  if (total == 0 || total < min_total)
    return NEAR_ALL;
  const int at = near_find(bins, n_bins, 0ull, near_target(total, frac));
  return at < 0 ? NEAR_ALL : (unsigned)at;
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

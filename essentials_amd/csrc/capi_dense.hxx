/**
 * @file capi_dense.hxx
 * @brief What the calls over dense feature matrices (grx_spmm, grx_spmm_values, grx_sddmm) share on the
 * host: the byte range of a strided matrix, whether it may be accessed 16 bytes at a time, and the
 * lanes a row of features takes.  Not installed.
 */
#pragma once

#include "capi_batch.hxx"

#include <gunrock/hip/kernels/spmm_kernels.hxx>

#include <cstdint>

namespace essentials_amd {

/// First to last element of a matrix of `rows` rows of F, `ld` apart: [first, last) in bytes.
struct byte_range_t {
  unsigned __int128 first, last;
  byte_range_t(const float* p, std::size_t rows, int64_t ld, int32_t F) {
    first = (std::uintptr_t)p;
    const unsigned __int128 elements = rows && F ? (unsigned __int128)(rows - 1) * (unsigned __int128)ld + F : 0;
    last = first + elements * sizeof(float);
  }
  bool empty() const { return last == first; }
  bool meets(const byte_range_t& o) const { return !empty() && !o.empty() && first < o.last && o.first < last; }
};

inline bool sixteen(const float* p, int64_t ld) { return (std::uintptr_t)p % 16 == 0 && ld % k::SPMM_VEC == 0; }

/// Lanes per row: the power of two that covers min(F, a tile) features at four per lane.
inline int lanes_for(int32_t F) {
  const int32_t quads = (std::min<int32_t>(F, k::SPMM_TILE) + k::SPMM_VEC - 1) / k::SPMM_VEC;
  int L = 1;
  while (L < quads)
    L *= 2;
  return L;
}

}  // namespace essentials_amd

/**
 * @file simple_csr.hxx
 * @brief The (row, column) keys of a CSR and what turns their sorted order into the simple graph
 * under it: shared by grx_graph_sorted_rows, grx_graph_simple (rmat.hip) and grx_truss, which builds
 * the same copy without weights and keeps it to itself.  Not installed.
 */
#pragma once

#include "capi_internal.hxx"

namespace essentials_amd {
namespace {

/// key[e] = (row << 32) | col for every edge: rows from the offsets by binary search
__global__ void __launch_bounds__(256)
    row_col_keys_kernel(const int* ap, const int* aj, int n_rows, long long nnz,
                        unsigned long long* keys) {
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < nnz; e += (long long)gridDim.x * 256) {
    int lo = 0, hi = n_rows;  // ap[lo] <= e < ap[hi]
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if ((long long)ap[mid] <= e)
        lo = mid;
      else
        hi = mid;
    }
    keys[e] = ((unsigned long long)(unsigned)lo << 32) | (unsigned)aj[e];
  }
}
__global__ void __launch_bounds__(256)
    keys_to_cols_kernel(const unsigned long long* keys, long long nnz, int* aj) {
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < nnz; e += (long long)gridDim.x * 256)
    aj[e] = (int)(unsigned)(keys[e] & 0xffffffffull);
}

/// 1 where entry e of the (row, column)-sorted keys stays in the simple graph: the first of its
/// run of repeats, and not a self loop.  e == nnz (the scan's total slot) -> 0.
struct simple_keep_t {
  const unsigned long long* keys;
  long long nnz;
  __host__ __device__ int operator()(long long e) const {
    if (e >= nnz)
      return 0;
    const unsigned long long key = keys[e];
    return (unsigned)(key >> 32) != (unsigned)key && (e == 0 || keys[e - 1] != key);
  }
};

/// Sorting keeps every row where it was: the new offset of a row is the kept entries before it.
__global__ void __launch_bounds__(256) simple_offsets_kernel(const int* ap, const int* at, int n_rows, int* ap_out) {
  for (long long r = blockIdx.x * 256ll + threadIdx.x; r <= n_rows; r += (long long)gridDim.x * 256)
    ap_out[r] = at[ap[r]];
}

}  // namespace
}  // namespace essentials_amd

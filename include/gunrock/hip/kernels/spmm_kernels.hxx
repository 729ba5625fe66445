/**
 * @file spmm_kernels.hxx
 * @brief Sparse-dense product Y = A X over weighted CSR rows (grx_spmm): features on the lanes,
 * a row's entries in time, every output element summed in a written order.
 *
 * A lane owns SPMM_VEC = 4 consecutive features and a group of L lanes owns one row, L the power of
 * two that covers min(F, SPMM_TILE) features; a wavefront holds 64 / L rows.  F above SPMM_TILE = 256
 * runs in feature tiles, blockIdx.y each.  The group walks the row's entries IN ROW ORDER: per entry
 * one load of X[c, f .. f + 3] per lane -- together the contiguous row of X -- and one fused
 * multiply-add per feature into an accumulator that started at 0.0f.  No sum crosses a lane, so the
 * order of an element's sum is the row's order whatever F, the leading dimensions or the grid are.
 *
 * Column id and weight are the same for the L lanes of a row: the group loads L entries with one
 * instruction each for ids and weights (lane j brings entry e0 + j), the next L while it works, and
 * hands them round (a lane read of the wavefront at L = 64, a shuffle within the group otherwise).
 * Below L = 4 (F <= 8) every lane reads the entries itself; the 1 or 2 lanes of a group share the
 * address.  SPMM_FLIGHT = 4 loads of X are in flight per lane ahead of the fma chain.
 *
 * A row of more than `segment` entries is cut by group_plan_kernel (group_rows.hxx) into items of
 * `segment` entries: spmm_gather_kernel leaves it out, spmm_segment_kernel sums one item per group
 * into partial[item * F + f], and spmm_combine_kernel adds a row's partial sums in segment order,
 * ((p0 + p1) + p2) + ..., one lane per (row, feature).  No float atomics.
 *
 * VEC says that X may be read 16 bytes at a time (base 16-byte aligned, ldx % 4 == 0): lanes whose
 * four features all lie below F then do, the lane of a ragged tail and every lane without VEC read
 * feature by feature.  vec_y says the same of a store target.  No access touches column F or beyond.
 * Offsets into X, Y and partial are 64-bit; entry offsets are the 32-bit values of ap[].
 */
#pragma once

#include <gunrock/hip/kernels/group_rows.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int SPMM_VEC = 4;      // features a lane owns
constexpr int SPMM_TILE = 256;   // features a wavefront covers at most: 64 lanes of 4
constexpr int SPMM_FLIGHT = 4;   // loads of X in flight per lane

/// The matrices of a call: row i of X begins at x + i * ldx, of Y at y + i * ldy; F features.
struct spmm_operands_t {
  const float* x;
  int64_t ldx;
  float* y;
  int64_t ldy;
  int32_t F;
  int32_t vec_y;  // y may be written 16 bytes at a time
};

/// Features [f, f + nf) of one row of X (nf <= 4; the others come back 0).
template <bool VEC>
__device__ __forceinline__ float4 spmm_load(const float* p, int nf) {
  if (VEC && nf == SPMM_VEC)
    return *reinterpret_cast<const float4*>(p);
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (nf > 0)
    v.x = p[0];
  if (nf > 1)
    v.y = p[1];
  if (nf > 2)
    v.z = p[2];
  if (nf > 3)
    v.w = p[3];
  return v;
}

/// The first nf of four sums to p; `vec`: p is 16-byte aligned.
__device__ __forceinline__ void spmm_store(float* p, const float4& v, int nf, bool vec) {
  if (vec && nf == SPMM_VEC) {
    *reinterpret_cast<float4*>(p) = v;
    return;
  }
  if (nf > 0)
    p[0] = v.x;
  if (nf > 1)
    p[1] = v.y;
  if (nf > 2)
    p[2] = v.z;
  if (nf > 3)
    p[3] = v.w;
}

/// Word `from` of the group's L lanes (from < L, the same in all of them).
template <int L>
__device__ __forceinline__ int32_t spmm_hand_round(int32_t word, int from) {
  if constexpr (L == wave_size)
    return __builtin_amdgcn_readlane(word, from);
  else
    return __shfl(word, from, L);
}

/**
 * @brief The sums over entries [lo, hi) of a lane's four features, entries in order, one fused
 * multiply-add each from 0.0f.  All L lanes of a group call it with the same range; `xf` is X
 * advanced to the lane's first feature and nf how many of its four lie below F (0: the lane only
 * helps to bring the entries).
 */
template <int L, bool VEC>
__device__ __forceinline__ float4 spmm_row_sum(const csr_rows_t& rows, const float* xf, int64_t ldx, int nf,
                                               int32_t lo, int32_t hi, int lane) {
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const auto step = [&](const int32_t (&c)[SPMM_FLIGHT], const float (&w)[SPMM_FLIGHT], uint32_t live) {
    float4 far[SPMM_FLIGHT];
#pragma unroll
    for (int k = 0; k < SPMM_FLIGHT; ++k) {
      far[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if ((uint32_t)k < live)
        far[k] = spmm_load<VEC>(xf + (int64_t)c[k] * ldx, nf);
    }
#pragma unroll
    for (int k = 0; k < SPMM_FLIGHT; ++k)
      if ((uint32_t)k < live) {
        acc.x = __fmaf_rn(far[k].x, w[k], acc.x);
        acc.y = __fmaf_rn(far[k].y, w[k], acc.y);
        acc.z = __fmaf_rn(far[k].z, w[k], acc.z);
        acc.w = __fmaf_rn(far[k].w, w[k], acc.w);
      }
  };
  // the walk counts in unsigned 32 bits, where e + L near the end of a CSR that fills its offsets cannot wrap
  const uint32_t end = (uint32_t)hi;
  if constexpr (L < SPMM_FLIGHT) {
    for (uint32_t e = (uint32_t)lo; e < end; e += SPMM_FLIGHT) {
      int32_t c[SPMM_FLIGHT];
      float w[SPMM_FLIGHT];
#pragma unroll
      for (int k = 0; k < SPMM_FLIGHT; ++k) {
        c[k] = 0;
        w[k] = 0.0f;
        if (e + k < end) {
          c[k] = rows.aj[e + k];
          w[k] = rows.ax[e + k];
        }
      }
      step(c, w, end - e);
    }
  } else {
    const auto bring = [&](uint32_t e0, int32_t& c, int32_t& w) {
      c = w = 0;
      if (e0 < end && e0 + lane < end) {
        c = rows.aj[e0 + lane];
        w = __float_as_int(rows.ax[e0 + lane]);
      }
    };
    int32_t mine_c, mine_w, next_c, next_w;
    bring((uint32_t)lo, mine_c, mine_w);
    for (uint32_t e0 = (uint32_t)lo; e0 < end; e0 += L) {
      bring(e0 + L, next_c, next_w);  // e0 < end <= 2^31 - 1 and L <= 64: no wrap
      const uint32_t count = min((uint32_t)L, end - e0);
      for (uint32_t k0 = 0; k0 < count; k0 += SPMM_FLIGHT) {
        int32_t c[SPMM_FLIGHT];
        float w[SPMM_FLIGHT];
#pragma unroll
        for (int k = 0; k < SPMM_FLIGHT; ++k) {  // L is a multiple of SPMM_FLIGHT: k0 + k < L
          c[k] = spmm_hand_round<L>(mine_c, (int)k0 + k);
          w[k] = __int_as_float(spmm_hand_round<L>(mine_w, (int)k0 + k));
        }
        step(c, w, count - k0);
      }
      mine_c = next_c;
      mine_w = next_w;
    }
  }
  return acc;
}

/// What a thread is within a launch: its group, its lane there, its features.
template <int L>
struct spmm_lane_t {
  int lane, nf;
  int64_t group, groups, f;
  __device__ __forceinline__ spmm_lane_t(int32_t F) {
    constexpr int PER_BLOCK = GROUP_BLOCK / L;
    lane = (int)threadIdx.x % L;
    group = (int64_t)blockIdx.x * PER_BLOCK + (int)threadIdx.x / L;
    groups = (int64_t)gridDim.x * PER_BLOCK;
    f = (int64_t)blockIdx.y * SPMM_TILE + lane * SPMM_VEC;
    nf = (int)max((int64_t)0, min((int64_t)SPMM_VEC, (int64_t)F - f));
  }
};

/// A wavefront-wide group walks a range it knows to be uniform.
template <int L>
__device__ __forceinline__ void spmm_uniform(int32_t& lo, int32_t& hi) {
  if constexpr (L == wave_size) {
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);
  }
}

/// Y[v, :] for every row of at most `segment` entries, a lane group each; gridDim.y feature tiles.
template <int L, bool VEC>
__global__ void __launch_bounds__(GROUP_BLOCK)
    spmm_gather_kernel(csr_rows_t rows, int32_t n, int32_t segment, spmm_operands_t m) {
  const spmm_lane_t<L> t(m.F);
  for (int64_t v = t.group; v < n; v += t.groups) {
    int32_t lo = rows.ap[v], hi = rows.ap[v + 1];
    spmm_uniform<L>(lo, hi);
    if (hi - lo > segment)  // spmm_combine_kernel writes the longer rows
      continue;
    const float4 acc = spmm_row_sum<L, VEC>(rows, m.x + t.f, m.ldx, t.nf, lo, hi, t.lane);
    spmm_store(m.y + v * m.ldy + t.f, acc, t.nf, m.vec_y != 0);
  }
}

/// partial[i * F + f] = the sums over item i of the long rows, a lane group each.
template <int L, bool VEC>
__global__ void __launch_bounds__(GROUP_BLOCK)
    spmm_segment_kernel(csr_rows_t rows, group_plan_t plan, int32_t segment, spmm_operands_t m, float* partial) {
  const spmm_lane_t<L> t(m.F);
  const int32_t n_items = min(plan.counts[1], plan.most_items);
  for (int64_t i = t.group; i < n_items; i += t.groups) {
    const int2 item = plan.items[i];
    const int64_t from = (int64_t)rows.ap[item.x] + (int64_t)item.y * segment;  // from + segment may pass 2^31
    int32_t lo = (int32_t)from, hi = (int32_t)min((int64_t)rows.ap[item.x + 1], from + segment);
    spmm_uniform<L>(lo, hi);
    const float4 acc = spmm_row_sum<L, VEC>(rows, m.x + t.f, m.ldx, t.nf, lo, hi, t.lane);
    spmm_store(partial + i * m.F + t.f, acc, t.nf, m.F % SPMM_VEC == 0);
  }
}

/// Y[v, f] of the long rows, a thread per element: the partial sums in segment order.
template <int header_only = 0>
__global__ void __launch_bounds__(GROUP_BLOCK)
    spmm_combine_kernel(csr_rows_t rows, group_plan_t plan, int32_t segment, spmm_operands_t m, const float* partial) {
  const int64_t elements = (int64_t)min(plan.counts[0], plan.most_rows) * m.F;
  for (int64_t at = (int64_t)blockIdx.x * GROUP_BLOCK + threadIdx.x; at < elements;
       at += (int64_t)gridDim.x * GROUP_BLOCK) {
    const int2 row = plan.rows[at / m.F];
    const int64_t f = at % m.F;
    const int32_t segments = (rows.ap[row.x + 1] - rows.ap[row.x] + segment - 1) / segment;
    if (row.y + segments > plan.most_items)  // sized from nnz, so it holds; it guards the reads all the same
      continue;
    float acc = partial[(int64_t)row.y * m.F + f];
    for (int32_t k = 1; k < segments; ++k)
      acc = __fadd_rn(acc, partial[(int64_t)(row.y + k) * m.F + f]);
    m.y[(int64_t)row.x * m.ldy + f] = acc;
  }
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

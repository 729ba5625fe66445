/**
 * @file sddmm_kernels.hxx
 * @brief Sampled dense-dense product out[e] = <U[row(e), :], V[col(e), :]> over the entries of a CSR
 * (grx_sddmm): features on the lanes, a row's entries in time, every dot product summed in a written
 * order.  The counterpart of spmm_kernels.hxx, whose gather of one row of a dense matrix per entry it
 * shares; there a lane keeps its own sums, here the lanes of a group meet once per entry.
 *
 * A lane owns SPMM_VEC = 4 consecutive features and a group of L lanes owns one row, L the power of
 * two that covers min(F, SPMM_TILE) features; a wavefront holds 64 / L rows.  The lane keeps its four
 * features of U[r] in registers for the whole row.  Column ids come in as in spmm_row_sum: lane j
 * brings entry e0 + j, the next L while the group works, and they are handed round (spmm_hand_round);
 * below L = 4 every lane reads the ids itself.  SPMM_FLIGHT = 4 entries are in flight: four loads of
 * V[c, f .. f + 3] per lane, then per entry the lane's partial p = fma(U[r, f], V[c, f], p) over its
 * features below F in ascending order from 0.0f.
 *
 * The order of a dot product (the contract of grx_sddmm): the partials of the L lanes meet in the
 * butterfly p[l] = p[l] + p[l ^ d], d = L / 2, L / 4, ..., 1, plain float32 adds.  Float32 addition
 * commutes bit for bit, so both lanes of a pair would compute the same sum; the four entries in flight
 * use that to share the wide stages (sddmm_meet): at d = L / 2 a lane sends the partials of two
 * entries and keeps the other two, at d = L / 4 it sends one and keeps one, and the stages below run
 * on one value.  3 + log2(L) - 2 exchanges serve four entries instead of 4 log2(L), and the result of
 * entry k ends in the lanes whose two upper bits are k; the first of them stores it, so a group
 * writes four consecutive floats with one instruction.
 *
 * F above SPMM_TILE = 256 (sddmm_tiles): a wavefront per row, tiles in ascending order inside the
 * walk; U's tile comes from memory again per four entries (it stays in the L1), the tile's partials
 * meet in the plain butterfly over the tile's own L (the last tile's may be below 64: stages d >= L
 * are left out, exactly as written), and tile sums are added in tile order, ((t0 + t1) + t2) + ...
 *
 * A row of more than `segment` entries is cut by group_plan_kernel (group_rows.hxx) into items of
 * `segment` entries: sddmm_rows_kernel leaves it out and sddmm_items_kernel gives an item to a group.
 * Entries are independent, so nothing is combined and `segment` cannot change a bit.  No atomics.
 *
 * VEC says that U and V may both be read 16 bytes at a time (bases 16-byte aligned, ldu % 4 == 0 and
 * ldv % 4 == 0): lanes whose four features all lie below F then do, the lane of a ragged tail and
 * every lane without VEC read feature by feature.  No access touches column F or beyond.  Offsets
 * into U and V are 64-bit; entry offsets are the 32-bit values of ap[].
 */
#pragma once

#include <gunrock/hip/kernels/spmm_kernels.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

/// The matrices of a call: row i of U begins at u + i * ldu, of V at v + i * ldv; out[nnz]; F features.
struct sddmm_operands_t {
  const float* u;
  int64_t ldu;
  const float* v;
  int64_t ldv;
  float* out;
  int32_t F;
};

/// A lane's partial: its nf features in ascending order, one fused multiply-add each from 0.0f.
__device__ __forceinline__ float sddmm_partial(const float4& u, const float4& v, int nf) {
  float p = 0.0f;
  if (nf > 0)
    p = __fmaf_rn(u.x, v.x, p);
  if (nf > 1)
    p = __fmaf_rn(u.y, v.y, p);
  if (nf > 2)
    p = __fmaf_rn(u.z, v.z, p);
  if (nf > 3)
    p = __fmaf_rn(u.w, v.w, p);
  return p;
}

/// a + (lane ^ d)'s b.
__device__ __forceinline__ float sddmm_pair(float a, float b, int d) {
  return __fadd_rn(a, __shfl_xor(b, d, wave_size));
}

/**
 * @brief The butterfly of four entries' partials over a group of L >= 4 lanes: returns the sum of
 * entry k = lane / (L / 4), the same bits p[k][l] + p[k][l ^ d], d = L / 2, ..., 1 leaves in any lane.
 */
template <int L>
__device__ __forceinline__ float sddmm_meet(const float (&p)[SPMM_FLIGHT], int lane) {
  static_assert(L >= 4 && SPMM_FLIGHT == 4, "two shared stages for four entries");
  constexpr int H = L / 2, Q = L / 4;
  const bool upper = (lane & H) != 0;  // keeps entries 2 and 3, sends 0 and 1
  const float a = sddmm_pair(upper ? p[2] : p[0], upper ? p[0] : p[2], H);
  const float b = sddmm_pair(upper ? p[3] : p[1], upper ? p[1] : p[3], H);
  const bool odd = (lane & Q) != 0;  // keeps b: entry 1 or 3
  float r = sddmm_pair(odd ? b : a, odd ? a : b, Q);
#pragma unroll
  for (int d = Q / 2; d > 0; d >>= 1)
    r = sddmm_pair(r, r, d);
  return r;
}

/**
 * @brief out[e] for the entries [lo, hi) of one row, F <= SPMM_TILE: all L lanes of a group call it
 * with the same range; `u` holds the lane's features of U[r], `vf` is V advanced to the lane's first
 * feature and nf how many of its four lie below F.
 */
template <int L, bool VEC>
__device__ __forceinline__ void sddmm_row(const int32_t* aj, const float4& u, const float* vf, int64_t ldv, int nf,
                                          int32_t lo, int32_t hi, int lane, float* out) {
  const auto partials = [&](const int32_t (&c)[SPMM_FLIGHT], uint32_t live, float (&p)[SPMM_FLIGHT]) {
    float4 far[SPMM_FLIGHT];
#pragma unroll
    for (int k = 0; k < SPMM_FLIGHT; ++k) {
      far[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if ((uint32_t)k < live)
        far[k] = spmm_load<VEC>(vf + (int64_t)c[k] * ldv, nf);
    }
#pragma unroll
    for (int k = 0; k < SPMM_FLIGHT; ++k)
      p[k] = (uint32_t)k < live ? sddmm_partial(u, far[k], nf) : 0.0f;
  };
  // the walk counts in unsigned 32 bits, where e + L near the end of a CSR that fills its offsets cannot wrap
  const uint32_t end = (uint32_t)hi;
  if constexpr (L < SPMM_FLIGHT) {
    for (uint32_t e = (uint32_t)lo; e < end; e += SPMM_FLIGHT) {
      int32_t c[SPMM_FLIGHT];
      float p[SPMM_FLIGHT];
#pragma unroll
      for (int k = 0; k < SPMM_FLIGHT; ++k)
        c[k] = e + k < end ? aj[e + k] : 0;
      const uint32_t live = end - e;
      partials(c, live, p);
      if constexpr (L == 1) {
#pragma unroll
        for (int k = 0; k < SPMM_FLIGHT; ++k)
          if ((uint32_t)k < live)
            out[e + k] = p[k];
      } else {  // two lanes: lane 0 ends with entries 0 and 1, lane 1 with 2 and 3
        const bool upper = lane != 0;
        const float a = sddmm_pair(upper ? p[2] : p[0], upper ? p[0] : p[2], 1);
        const float b = sddmm_pair(upper ? p[3] : p[1], upper ? p[1] : p[3], 1);
        const uint32_t k = upper ? 2 : 0;
        if (k < live)
          out[e + k] = a;
        if (k + 1 < live)
          out[e + k + 1] = b;
      }
    }
  } else {
    const auto bring = [&](uint32_t e0) {
      return e0 < end && e0 + lane < end ? aj[e0 + lane] : 0;
    };
    int32_t mine = bring((uint32_t)lo);
    for (uint32_t e0 = (uint32_t)lo; e0 < end; e0 += L) {
      const int32_t next = bring(e0 + L);  // e0 < end <= 2^31 - 1 and L <= 64: no wrap
      const uint32_t count = min((uint32_t)L, end - e0);
      for (uint32_t k0 = 0; k0 < count; k0 += SPMM_FLIGHT) {
        int32_t c[SPMM_FLIGHT];
        float p[SPMM_FLIGHT];
#pragma unroll
        for (int k = 0; k < SPMM_FLIGHT; ++k)  // L is a multiple of SPMM_FLIGHT: k0 + k < L
          c[k] = spmm_hand_round<L>(mine, (int)k0 + k);
        const uint32_t live = count - k0;
        partials(c, live, p);
        const float r = sddmm_meet<L>(p, lane);
        const uint32_t k = (uint32_t)lane / (L / 4);
        if (lane % (L / 4) == 0 && k < live)
          out[e0 + k0 + k] = r;
      }
      mine = next;
    }
  }
}

/**
 * @brief out[e] for the entries [lo, hi) of one row, F > SPMM_TILE: a whole wavefront calls it with
 * the same range; `ur` is U[r] and `v` the matrix V.
 */
template <bool VEC>
__device__ __forceinline__ void sddmm_tiles(const int32_t* aj, const float* ur, const float* v, int64_t ldv, int32_t F,
                                            int32_t lo, int32_t hi, int lane, float* out) {
  constexpr int L = wave_size;
  const uint32_t end = (uint32_t)hi;
  const auto bring = [&](uint32_t e0) {
    return e0 < end && e0 + lane < end ? aj[e0 + lane] : 0;
  };
  int32_t mine = bring((uint32_t)lo);
  for (uint32_t e0 = (uint32_t)lo; e0 < end; e0 += L) {
    const int32_t next = bring(e0 + L);
    const uint32_t count = min((uint32_t)L, end - e0);
    for (uint32_t k0 = 0; k0 < count; k0 += SPMM_FLIGHT) {
      const uint32_t live = count - k0;
      int32_t c[SPMM_FLIGHT];
      float sum[SPMM_FLIGHT];
#pragma unroll
      for (int k = 0; k < SPMM_FLIGHT; ++k) {
        c[k] = spmm_hand_round<L>(mine, (int)k0 + k);
        sum[k] = 0.0f;
      }
      for (int32_t f0 = 0; f0 < F; f0 += SPMM_TILE) {
        // the tile's own group width: the power of two that covers its features at four per lane
        const int32_t quads = (min(F - f0, (int32_t)SPMM_TILE) + SPMM_VEC - 1) / SPMM_VEC;
        int width = 1;
        while (width < quads)
          width *= 2;
        const int64_t f = (int64_t)f0 + lane * SPMM_VEC;
        const int nf = (int)max((int64_t)0, min((int64_t)SPMM_VEC, (int64_t)F - f));
        const float4 u = spmm_load<VEC>(ur + f, nf);
        float4 far[SPMM_FLIGHT];
#pragma unroll
        for (int k = 0; k < SPMM_FLIGHT; ++k) {
          far[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          if ((uint32_t)k < live)
            far[k] = spmm_load<VEC>(v + (int64_t)c[k] * ldv + f, nf);
        }
#pragma unroll
        for (int k = 0; k < SPMM_FLIGHT; ++k) {
          float p = sddmm_partial(u, far[k], nf);
#pragma unroll
          for (int d = L / 2; d > 0; d >>= 1) {
            const float met = sddmm_pair(p, p, d);  // every lane takes part in the exchange
            if (d < width)
              p = met;
          }
          sum[k] = f0 == 0 ? p : __fadd_rn(sum[k], p);
        }
      }
      // lane 0 belongs to every tile's group: its sums are the results; lanes 0 to 3 store one each
      float r = 0.0f;
#pragma unroll
      for (int k = 0; k < SPMM_FLIGHT; ++k) {
        const float s = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sum[k])));
        if (lane == k)
          r = s;
      }
      if ((uint32_t)lane < min(live, (uint32_t)SPMM_FLIGHT))
        out[e0 + k0 + lane] = r;
    }
    mine = next;
  }
}

/// The entries [lo, hi) of row r by one lane group.
template <int L, bool VEC, bool TILED>
__device__ __forceinline__ void sddmm_range(const int32_t* aj, const sddmm_operands_t& m, int64_t r, int32_t lo,
                                            int32_t hi, const spmm_lane_t<L>& t) {
  if constexpr (TILED) {
    sddmm_tiles<VEC>(aj, m.u + r * m.ldu, m.v, m.ldv, m.F, lo, hi, t.lane, m.out);
  } else {
    const float4 u = spmm_load<VEC>(m.u + r * m.ldu + t.f, t.nf);
    sddmm_row<L, VEC>(aj, u, m.v + t.f, m.ldv, t.nf, lo, hi, t.lane, m.out);
  }
}

/// out[e] for the entries of every row of at most `segment` entries, a lane group each.
template <int L, bool VEC, bool TILED>
__global__ void __launch_bounds__(GROUP_BLOCK)
    sddmm_rows_kernel(csr_rows_t rows, int32_t n, int32_t segment, sddmm_operands_t m) {
  static_assert(!TILED || L == wave_size, "feature tiles take a wavefront per row");
  const spmm_lane_t<L> t(m.F);
  for (int64_t v = t.group; v < n; v += t.groups) {
    int32_t lo = rows.ap[v], hi = rows.ap[v + 1];
    spmm_uniform<L>(lo, hi);
    if (hi - lo > segment || hi <= lo)  // sddmm_items_kernel writes the longer rows
      continue;
    sddmm_range<L, VEC, TILED>(rows.aj, m, v, lo, hi, t);
  }
}

/// out[e] for the entries of item i of the long rows, a lane group each.
template <int L, bool VEC, bool TILED>
__global__ void __launch_bounds__(GROUP_BLOCK)
    sddmm_items_kernel(csr_rows_t rows, group_plan_t plan, int32_t segment, sddmm_operands_t m) {
  static_assert(!TILED || L == wave_size, "feature tiles take a wavefront per row");
  const spmm_lane_t<L> t(m.F);
  const int32_t n_items = min(plan.counts[1], plan.most_items);
  for (int64_t i = t.group; i < n_items; i += t.groups) {
    const int2 item = plan.items[i];
    const int64_t from = (int64_t)rows.ap[item.x] + (int64_t)item.y * segment;  // from + segment may pass 2^31
    int32_t lo = (int32_t)from, hi = (int32_t)min((int64_t)rows.ap[item.x + 1], from + segment);
    spmm_uniform<L>(lo, hi);
    sddmm_range<L, VEC, TILED>(rows.aj, m, item.x, lo, hi, t);
  }
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

/**
 * @file bc_kernels.hxx
 * @brief Betweenness centrality's two sweeps over a BFS's level lists (grx_bc).
 *
 * The reference (algorithms/bc.hxx) pushes sigma and delta with one float atomic per edge, so its
 * sums depend on the order the atomics land in.  Here both sweeps PULL: a row of level d sums over
 * its own neighbours one level up (forward, in-edges) or down (backward, out-edges), and every sum
 * is taken in a fixed order -- the same call returns the same bits:
 *   - rows shorter than BC_HUB: BC_GROUP (16) lanes share a row, each lane adds its strided
 *     edges in edge order, a 4-step shuffle tree combines them;
 *   - longer rows are cut into chunks of BC_CHUNK edges (chunk k covers edges [k, k + 1) *
 *     BC_CHUNK of the row); bc_hub_chunk_kernel writes every chunk's sum to its own slot, and the
 *     row's group adds its slots in chunk order -- the deterministic counterpart of
 *     hub_chunk_sum_kernel (reduce_kernels.hxx), which adds chunks atomically.
 *
 * Positions p index the level list `verts` (reached vertices ordered by depth); `chunk_start`
 * is the exclusive scan of the rows' chunk counts over positions, so position p owns the chunk
 * slots [chunk_start[p], chunk_start[p + 1]).
 * Forward, level d:  sigma[v] = sum over in-edges (u -> v), depth[u] == d - 1, of sigma[u]
 *                    (level 1: every such u is the source, sigma = 1); rho[v] = 1 / sigma[v].
 * Backward, level d: s = sum over out-edges (u -> w), depth[w] == d + 1, of rho[w];
 *                    delta[u] = sigma[u] * s;  rho[u] = (1 + delta[u]) / sigma[u];
 *                    bc[u] += 0.5 * delta[u].
 * rho[w] = (1 + delta[w]) / sigma[w] is what an edge into w contributes per unit of sigma[u], so
 * the backward sweep gathers one word per edge; level D-1 keeps the forward sweep's 1 / sigma.
 *
 * The arithmetic as compiled for gfx950 (floating-point contraction is on by default):
 *   - delta[u] = fl(sigma[u] * s), the rounded product, and bc[u] = fl(bc[u] + 0.5 * delta[u]);
 *   - rho[u] = fl(fma(sigma[u], s, 1) / sigma[u]): the product is NOT rounded before the 1 is
 *     added, so the numerator is fl(1 + sigma[u] * s), not fl(1 + delta[u]) -- the two differ by
 *     at most one rounding, and not at all when the product is exact;
 *   - both divisions are the correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence,
 *     denormals kept.
 * Every term of every sum is non-negative, so a sum of c terms taken in any order (zeros of empty
 * lanes and chunks included) is within c - 1 roundings of the exact sum of its rounded terms: the
 * relative error of bc[v] grows with the number of roundings on the paths through v, not with
 * max |bc|.  tests/bc_oracle.py counts them and models the three lines above.
 * Path counts above FLT_MAX (sigma = inf) and reciprocals below the normal range are outside the
 * contract, as they are for the reference's float atomics.
 */
#pragma once

#include <gunrock/hip/primitives.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int BC_BLOCK = 256;
constexpr int BC_GROUP = 16;          // lanes per row
constexpr int BC_HUB = 256;           // rows at least this long are summed in chunks ...
constexpr int BC_CHUNK = 2048;        // ... of this many edges

/// Chunks of a row whose in- and out-degree are `in_deg` / `out_deg` (both sweeps use the same
/// slots: a chunk past the end of one direction's row sums nothing).
__host__ __device__ __forceinline__ int bc_chunks_of(int in_deg, int out_deg) {
  const int deg = in_deg > out_deg ? in_deg : out_deg;
  return deg >= BC_HUB ? (deg + BC_CHUNK - 1) / BC_CHUNK : 0;
}

/// Level boundaries of the sorted keys (key = depth, `cap` = unreached): offsets[d] = first
/// position whose key is >= d, for d = 0 .. cap.  counters[0] += reached vertices, counters[1] +=
/// the sum of their out-degrees.
__global__ void __launch_bounds__(BC_BLOCK)
    bc_level_bounds_kernel(const unsigned* __restrict__ keys, const int32_t* __restrict__ verts,
                           const int32_t* __restrict__ ap, int32_t n, unsigned cap,
                           int32_t* __restrict__ offsets, unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long s_v[BC_BLOCK / wave_size], s_e[BC_BLOCK / wave_size];
  unsigned long long reached = 0, edges = 0;
  for (int32_t p = blockIdx.x * BC_BLOCK + threadIdx.x; p < n; p += gridDim.x * BC_BLOCK) {
    const unsigned k = keys[p];
    const unsigned before = p ? keys[p - 1] + 1u : 0u;
    for (unsigned d = before; d <= k; ++d)
      offsets[d] = p;
    if (p == n - 1)
      for (unsigned d = k + 1; d <= cap; ++d)
        offsets[d] = n;
    if (k < cap) {
      const int32_t v = verts[p];
      ++reached;
      edges += (unsigned long long)(ap[v + 1] - ap[v]);
    }
  }
  reached = wave_sum(reached);
  edges = wave_sum(edges);
  if (lane_id() == 0) {
    s_v[threadIdx.x / wave_size] = reached;
    s_e[threadIdx.x / wave_size] = edges;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long tv = 0, te = 0;
#pragma unroll
    for (int w = 0; w < BC_BLOCK / wave_size; ++w) {
      tv += s_v[w];
      te += s_e[w];
    }
    if (tv)
      atomicAdd(&counters[0], tv);  // integer sums: their order does not matter
    if (te)
      atomicAdd(&counters[1], te);
  }
}

/// hub_start[d] = chunk_start[offsets[d]], d = 0 .. cap: the first chunk slot of level d.
__global__ void __launch_bounds__(BC_BLOCK)
    bc_hub_bounds_kernel(const int32_t* __restrict__ offsets, const int32_t* __restrict__ chunk_start,
                         unsigned cap, int32_t* __restrict__ hub_start) {
  for (unsigned d = blockIdx.x * BC_BLOCK + threadIdx.x; d <= cap; d += gridDim.x * BC_BLOCK)
    hub_start[d] = chunk_start[offsets[d]];
}

/// owner[c] = the position whose row chunk slot c belongs to, for every slot of positions [0, n).
__global__ void __launch_bounds__(BC_BLOCK)
    bc_chunk_owner_kernel(const int32_t* __restrict__ chunk_start, int32_t n, int32_t* __restrict__ owner) {
  for (int32_t p = blockIdx.x * BC_BLOCK + threadIdx.x; p < n; p += gridDim.x * BC_BLOCK)
    for (int32_t c = chunk_start[p], end = chunk_start[p + 1]; c < end; ++c)
      owner[c] = p;
}

/// One chunk of a hub row per workgroup trip: partial[c] = the chunk's sum (fixed order: each
/// thread adds its strided edges in order, then the wave tree, then the waves in order).  The
/// level's chunk slots are [c_lo, c_lo + n_chunks); owner[c] is the position of slot c's row.
template <bool FORWARD>
__global__ void __launch_bounds__(BC_BLOCK)
    bc_hub_chunk_kernel(const int32_t* __restrict__ ap, const int32_t* __restrict__ aj,
                        const int32_t* __restrict__ verts, const int32_t* __restrict__ chunk_start,
                        const int32_t* __restrict__ owner, int32_t c_lo, int32_t n_chunks,
                        const int32_t* __restrict__ depth, int32_t want, const float* __restrict__ val,
                        float* __restrict__ partial) {
  __shared__ float s_part[BC_BLOCK / wave_size];
  const bool unit = FORWARD && want == 0;  // forward level 1: the only neighbour one level up is the source
  for (int32_t c = c_lo + (int32_t)blockIdx.x; c < c_lo + n_chunks; c += (int32_t)gridDim.x) {
    const int32_t lo = owner[c];  // the hub's position (a binary search here cost 22 dependent loads)
    const int32_t v = verts[lo];
    const int32_t row_end = ap[v + 1];
    const int64_t first64 = (int64_t)ap[v] + (int64_t)(c - chunk_start[lo]) * BC_CHUNK;
    const int32_t count = first64 < row_end ? (int32_t)std::min<int64_t>(row_end - first64, BC_CHUNK) : 0;
    const int32_t first = (int32_t)std::min<int64_t>(first64, row_end);
    float sum = 0.f;
    for (int32_t j = threadIdx.x; j < count; j += BC_BLOCK) {
      const int32_t u = aj[first + j];
      if (depth[u] == want)
        sum += unit ? 1.f : val[u];
    }
    sum = wave_sum(sum);
    if (lane_id() == 0)
      s_part[threadIdx.x / wave_size] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      float total = 0.f;
#pragma unroll
      for (int w = 0; w < BC_BLOCK / wave_size; ++w)
        total += s_part[w];
      partial[c] = total;
    }
    __syncthreads();  // s_part is rewritten by the next chunk
  }
}

/// One level of a sweep: positions [p_lo, p_lo + n) of the level list, BC_GROUP lanes per row.
/// FORWARD: (ap, aj) are the in-edges, want = d - 1, val = sigma.  Backward: the out-edges,
/// want = d + 1, val = rho.  Hub rows add the slots bc_hub_chunk_kernel wrote for them.
template <bool FORWARD>
__global__ void __launch_bounds__(BC_BLOCK)
    bc_level_kernel(const int32_t* __restrict__ ap, const int32_t* __restrict__ aj,
                    const int32_t* __restrict__ verts, const int32_t* __restrict__ chunk_start,
                    const float* __restrict__ partial, int32_t p_lo, int32_t n,
                    const int32_t* __restrict__ depth, int32_t want, const float* val,
                    float* sigma, float* rho, float* __restrict__ bc) {
  const int lane = threadIdx.x & (BC_GROUP - 1);
  const bool unit = FORWARD && want == 0;
  const int32_t groups = (int32_t)gridDim.x * (BC_BLOCK / BC_GROUP);
  // every wavefront makes the same number of trips: the shuffles below need all 64 lanes
  const int32_t trips = (n + groups - 1) / groups;
  int32_t row = (int32_t)((blockIdx.x * BC_BLOCK + threadIdx.x) / BC_GROUP);
  for (int32_t t = 0; t < trips; ++t, row += groups) {
    float sum = 0.f;
    int32_t v = 0;
    if (row < n) {
      const int32_t p = p_lo + row;
      v = verts[p];
      const int32_t c0 = chunk_start[p], c1 = chunk_start[p + 1];
      if (c1 > c0) {
        if (lane == 0)
          for (int32_t c = c0; c < c1; ++c)
            sum += partial[c];
      } else {
        const int32_t first = ap[v], deg = ap[v + 1] - first;
        for (int32_t j = lane; j < deg; j += BC_GROUP) {
          const int32_t u = aj[first + j];
          if (depth[u] == want)  // the depth first: most neighbours are not one level away
            sum += unit ? 1.f : val[u];
        }
      }
    }
#pragma unroll
    for (int d = BC_GROUP / 2; d > 0; d >>= 1)
      sum += __shfl_xor(sum, d, BC_GROUP);
    if (row < n && lane == 0) {
      if (FORWARD) {
        sigma[v] = sum;
        rho[v] = 1.f / sum;
      } else {
        const float s = sigma[v];
        const float delta = s * sum;
        rho[v] = (1.f + delta) / s;
        bc[v] += 0.5f * delta;
      }
    }
  }
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

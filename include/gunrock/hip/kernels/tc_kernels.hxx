/**
 * @file tc_kernels.hxx
 * @brief Triangle counting (grx_tc): the degree-oriented copy L of a symmetric CSR and the
 * intersections on it.
 *
 * L keeps entry v of row u iff v != u, v is not a repeat of the row, and rank(u) < rank(v), where
 * rank orders vertices by (row length, id).  Every triangle {u, v, w} with rank u < v < w is then
 * found exactly once, at u: v and w both lie in out(u), and w lies in out(v).  Rows of L are sorted
 * by column, and no row of L is longer than sqrt(nnz).
 *
 * Building L (wave per row, ballot compaction):
 *   tc_orient_kernel<false>  kept entries per row;  exclusive scan -> K;
 *   tc_orient_kernel<true>   key (u << bits) | v at K[u] + rank;  radix sort of the keys;
 *   tc_distinct_kernel<...>  the same two steps over the sorted keys, dropping repeats -> L.
 *
 * Counting at u, for every 2-path u -> v -> w (the "probes"), flattened over the workers of u:
 * worker t finds v_i by a binary search of the inclusive prefix of out-degrees over out(u), reads
 * w = out(v_i)[t - prefix], and binary-searches w in out(u).  A hit adds one to slot i (v) and slot
 * j (w) -- 32-bit counters beside out(u) -- and one to u's total.  The slots and u's total go to
 * the int64 per-vertex output once per oriented edge, by integer atomics (order-free).
 *   tc_group_kernel<G>:       rows of at most G entries, G lanes each (G = 8 or 64), in LDS;
 *   tc_block_kernel<true>:    one workgroup per row, out(u) staged in dynamic LDS (16 B per id);
 *   tc_block_kernel<false>:   rows longer than the staging capacity: one workgroup per row, the
 *                             row of L itself is searched in global memory and the prefix, base
 *                             and counter slots live in a global workspace at L's positions (the
 *                             counters take global atomics there: this path is for the few rows
 *                             that do not fit).
 */
#pragma once

#include <gunrock/hip/primitives.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int TC_BLOCK = 256;
constexpr int TC_SMALL = 8;        // rows of L with at most this many entries: 8 lanes each
constexpr int TC_WAVE = 64;        // ... at most this many: one wavefront each
constexpr int TC_MEDIUM = 1024;    // ... at most this many: one workgroup each, 16 KB of LDS
constexpr int TC_LDS_IDS = 8192;   // default staging capacity of the workgroup path (128 KB)
constexpr int TC_SLOT_BYTES = 16;  // per staged id: id, inclusive prefix, base, counter
constexpr int TC_CLASSES = 6;      // <2 entries (nothing to find), group 8, group 64, medium, large, global

/// rank(u) < rank(v): vertices ordered by (row length, id).  du = row length of u.
__device__ __forceinline__ bool tc_before(const int32_t* ap, int32_t u, int32_t du, int32_t v) {
  const int32_t dv = ap[v + 1] - ap[v];
  return du < dv || (du == dv && u < v);
}

/// Oriented entries of each row of the CSR (!WRITE: count[u]), or their keys at at[u] (WRITE).
template <bool WRITE>
__global__ void __launch_bounds__(TC_BLOCK)
    tc_orient_kernel(const int32_t* ap, const int32_t* aj, int32_t n, int32_t* count, const int32_t* at,
                     unsigned long long* keys, int bits) {
  constexpr int WAVES = TC_BLOCK / wave_size;
  const int lane = lane_id();
  const int64_t stride = (int64_t)gridDim.x * WAVES;
  for (int64_t u = (int64_t)blockIdx.x * WAVES + threadIdx.x / wave_size; u < n; u += stride) {
    const int32_t lo = ap[u], hi = ap[u + 1], du = hi - lo;
    int32_t out = WRITE ? at[u] : 0;
    for (int32_t e0 = lo; e0 < hi; e0 += wave_size) {
      const int32_t e = e0 + lane;
      bool keep = false;
      int32_t v = 0;
      if (e < hi) {
        v = aj[e];
        keep = v != (int32_t)u && tc_before(ap, (int32_t)u, du, v);
      }
      const unsigned long long m = __ballot(keep);
      if (WRITE && keep)
        keys[out + rank_in_mask(m)] = ((unsigned long long)u << bits) | (unsigned)v;
      out += __popcll(m);
    }
    if (!WRITE && lane == 0)
      count[u] = out;
  }
}

/// Over the sorted keys (row u at [K[u], K[u + 1])): distinct entries per row (!WRITE: count[u]),
/// or their columns at at[u] (WRITE).
template <bool WRITE>
__global__ void __launch_bounds__(TC_BLOCK)
    tc_distinct_kernel(const unsigned long long* keys, const int32_t* K, int32_t n, int32_t* count,
                       const int32_t* at, int32_t* cols, unsigned long long col_mask) {
  constexpr int WAVES = TC_BLOCK / wave_size;
  const int lane = lane_id();
  const int64_t stride = (int64_t)gridDim.x * WAVES;
  for (int64_t u = (int64_t)blockIdx.x * WAVES + threadIdx.x / wave_size; u < n; u += stride) {
    const int32_t lo = K[u], hi = K[u + 1];
    int32_t out = WRITE ? at[u] : 0;
    for (int32_t e0 = lo; e0 < hi; e0 += wave_size) {
      const int32_t e = e0 + lane;
      bool keep = false;
      unsigned long long key = 0;
      if (e < hi) {
        key = keys[e];
        keep = e == lo || keys[e - 1] != key;
      }
      const unsigned long long m = __ballot(keep);
      if (WRITE && keep)
        cols[out + rank_in_mask(m)] = (int32_t)(key & col_mask);
      out += __popcll(m);
    }
    if (!WRITE && lane == 0)
      count[u] = out;
  }
}

/// Size class of a row of L with d entries (bounds b[0..3] = group 8, group 64, medium, capacity).
__host__ __device__ __forceinline__ unsigned tc_class_of(int32_t d, const int32_t* b) {
  return d < 2 ? 0u : d <= b[0] ? 1u : d <= b[1] ? 2u : d <= b[2] ? 3u : d <= b[3] ? 4u : 5u;
}

/// starts[c] = first position of class c in the class-sorted keys (c = 0 .. TC_CLASSES).
__global__ void tc_class_starts_kernel(const unsigned* keys, int32_t n, int32_t* starts) {
  const int c = threadIdx.x;
  if (c > TC_CLASSES)
    return;
  int32_t lo = 0, hi = n;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (keys[mid] < (unsigned)c)
      lo = mid + 1;
    else
      hi = mid;
  }
  starts[c] = lo;
}

/// Position of w in the sorted id[0, d), or -1.
__device__ __forceinline__ int32_t tc_find(const int32_t* id, int32_t d, int32_t w) {
  int32_t lo = 0, hi = d;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (id[mid] < w)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < d && id[lo] == w ? lo : -1;
}

/// Triangles and probes of the whole launch: one atomic pair per wavefront.
__device__ __forceinline__ void tc_flush_totals(unsigned long long tri, unsigned long long probes,
                                                unsigned long long* totals) {
  tri = wave_sum(tri);
  probes = wave_sum(probes);
  if (lane_id() == 0) {
    if (tri)
      atomicAdd(&totals[0], tri);
    if (probes)
      atomicAdd(&totals[1], probes);
  }
}

/// Rows of L with 2 .. G entries, G lanes each (TC_BLOCK / G rows per workgroup and batch).
/// counts: int64[V] (as unsigned long long) or nullptr; totals: [triangles, probes].
template <int G>
__global__ void __launch_bounds__(TC_BLOCK)
    tc_group_kernel(const int32_t* lap, const int32_t* laj, const int32_t* rows, int32_t n_rows,
                    unsigned long long* counts, unsigned long long* totals) {
  static_assert(G <= wave_size && TC_BLOCK % G == 0, "a row's lanes lie in one wavefront");
  constexpr int GROUPS = TC_BLOCK / G;
  __shared__ int32_t s_id[TC_BLOCK], s_pre[TC_BLOCK], s_base[TC_BLOCK], s_cnt[TC_BLOCK];
  const int l = threadIdx.x % G;
  const int first = threadIdx.x - l;
  int32_t* id = s_id + first;
  int32_t* pre = s_pre + first;
  int32_t* base = s_base + first;
  int32_t* cnt = s_cnt + first;
  unsigned long long tri = 0, probes = 0;
  // every group of the workgroup runs the same number of batches: the barriers are uniform
  for (int64_t r0 = (int64_t)blockIdx.x * GROUPS; r0 < n_rows; r0 += (int64_t)gridDim.x * GROUPS) {
    const int64_t r = r0 + threadIdx.x / G;
    int32_t u = 0, d = 0, lo = 0;
    if (r < n_rows) {
      u = rows[r];
      lo = lap[u];
      d = lap[u + 1] - lo;
    }
    int32_t v = 0, start = 0, dv = 0;
    if (l < d) {
      v = laj[lo + l];
      start = lap[v];
      dv = lap[v + 1] - start;
    }
    int32_t incl = dv;
#pragma unroll
    for (int k = 1; k < G; k <<= 1) {
      const int32_t y = __shfl_up(incl, k, G);
      if (l >= k)
        incl += y;
    }
    id[l] = v;
    pre[l] = incl;
    base[l] = start - (incl - dv);
    cnt[l] = 0;
    const int32_t P = __shfl(incl, d > 0 ? d - 1 : 0, G);
    __syncthreads();
    unsigned mine = 0;
    for (int32_t t = l; t < P; t += G) {
      const int32_t i = prefix_owner(pre, d, t);
      const int32_t j = tc_find(id, d, laj[base[i] + t]);
      if (j >= 0) {
        ++mine;
        if (counts) {
          atomicAdd(&cnt[i], 1);
          atomicAdd(&cnt[j], 1);
        }
      }
    }
    tri += mine;
    if (l == 0)
      probes += (unsigned long long)P;
    unsigned long long tu = mine;
#pragma unroll
    for (int k = G / 2; k > 0; k >>= 1)
      tu += __shfl_xor(tu, k, G);
    __syncthreads();
    // each lane flushes (and next batch rewrites) only its own slot
    if (counts) {
      if (l < d && cnt[l])
        atomicAdd(&counts[id[l]], (unsigned long long)cnt[l]);
      if (l == 0 && tu)
        atomicAdd(&counts[u], tu);
    }
  }
  tc_flush_totals(tri, probes, totals);
}

/// One workgroup per row of L.  STAGED: out(u) and its slots in dynamic LDS (cap ids, 16 B
/// each).  !STAGED: the row is read in place and its slots are ws[0 | m | 2m + L's positions].
template <bool STAGED>
__global__ void __launch_bounds__(TC_BLOCK)
    tc_block_kernel(const int32_t* lap, const int32_t* laj, const int32_t* rows, int32_t n_rows, int32_t cap,
                    int32_t* ws, int64_t m, unsigned long long* counts, unsigned long long* totals) {
  extern __shared__ int32_t s_dyn[];
  __shared__ int32_t s_wave[TC_BLOCK / wave_size + 1];
  __shared__ unsigned long long s_tri[TC_BLOCK / wave_size];
  const int tid = threadIdx.x;
  unsigned long long tri = 0, probes = 0;
  for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const int32_t u = rows[r];
    const int32_t lo = lap[u], d = lap[u + 1] - lo;
    const int32_t* id;
    int32_t *sid, *pre, *base, *cnt;
    if constexpr (STAGED) {
      sid = s_dyn;
      pre = s_dyn + cap;
      base = s_dyn + 2 * (int64_t)cap;
      cnt = s_dyn + 3 * (int64_t)cap;
      id = sid;
    } else {
      sid = nullptr;
      pre = ws + lo;
      base = ws + m + lo;
      cnt = ws + 2 * m + lo;
      id = laj + lo;
    }
    // stage: each thread a contiguous chunk, local inclusive prefix, then the workgroup's scan
    const int32_t per = (d + TC_BLOCK - 1) / TC_BLOCK;
    const int32_t c0 = min(d, tid * per), c1 = min(d, c0 + per);
    int32_t run = 0;
    for (int32_t i = c0; i < c1; ++i) {
      const int32_t v = laj[lo + i];
      const int32_t start = lap[v];
      if constexpr (STAGED)
        sid[i] = v;
      base[i] = start - run;
      run += lap[v + 1] - start;
      pre[i] = run;
      cnt[i] = 0;
    }
    int32_t P = 0;
    const int32_t offset = block_exclusive_sum<TC_BLOCK>(run, P, s_wave);
    for (int32_t i = c0; i < c1; ++i) {
      pre[i] += offset;
      base[i] -= offset;
    }
    __syncthreads();
    unsigned mine = 0;
    for (int32_t t = tid; t < P; t += TC_BLOCK) {
      const int32_t i = prefix_owner(pre, d, t);
      const int32_t j = tc_find(id, d, laj[base[i] + t]);
      if (j >= 0) {
        ++mine;
        if (counts) {
          atomicAdd(&cnt[i], 1);
          atomicAdd(&cnt[j], 1);
        }
      }
    }
    tri += mine;
    if (tid == 0)
      probes += (unsigned long long)P;
    const unsigned long long tw = wave_sum((unsigned long long)mine);
    if (lane_id() == 0)
      s_tri[tid / wave_size] = tw;
    __syncthreads();
    if (counts) {
      for (int32_t i = tid; i < d; i += TC_BLOCK)
        if (cnt[i])
          atomicAdd(&counts[id[i]], (unsigned long long)cnt[i]);
      if (tid == 0) {
        unsigned long long tu = 0;
        for (int w = 0; w < TC_BLOCK / wave_size; ++w)
          tu += s_tri[w];
        if (tu)
          atomicAdd(&counts[u], tu);
      }
    }
    __syncthreads();  // the next row restages the slots and s_tri
  }
  tc_flush_totals(tri, probes, totals);
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

/**
 * @file spgemm_kernels.hxx
 * @brief Sparse matrix product C = A * B (grx_spgemm): two-phase Gustavson, one row of C per group
 * of lanes, the row's columns accumulated in LDS.
 *
 * Row i of C is the union over the entries (i, k) of row i of A of row k of B; every pair is one
 * PRODUCT.  u(i), the products of row i, bounds its entries, and so does B's column count.
 *
 *   spgemm_bound_kernel           u(i) in 64 bits and min(u(i), n_cols), a wavefront per row;
 *   spgemm_group_kernel<G, NUM>   rows of few products (G = 8 lanes, 64 slots) or few entries
 *                                 (G = 64 lanes, 512 slots): an open-addressing table per group in
 *                                 static LDS, atomicCAS on the 4-byte key, -1 = empty, linear probing;
 *   spgemm_block_kernel<NUM>      one workgroup per row, the table in dynamic LDS, its capacity the
 *                                 power of two >= 2 * (bound or exact entries) of THAT row, so that
 *                                 clearing and sorting cost what the row needs and no more;
 *   spgemm_dense_kernel<NUM>      rows no table holds at load factor 1/2: one workgroup per row walks
 *                                 the row's products once per TILE of columns, with a bitmap (and a
 *                                 float per column) of the tile in dynamic LDS.
 *
 * NUM = false is the symbolic phase (count the distinct columns), NUM = true the numeric one: a float
 * beside each key takes the products by LDS atomicAdd, the table is then sorted in place by a
 * bitonic network on (unsigned key, value) -- the empty key 0xffffffff sorts last -- and its first
 * entries are the row of C.  A tile's bitmap is read out in column order, which is sorted already.
 *
 * Why the dense path is a tile in LDS and not a strip in global memory: a strip shared by the
 * threads of a workgroup needs float atomics to global memory for the sums, which this call does
 * not use.  The price is one walk over the row's products per tile: ceil(n_cols / tile) of them,
 * with about 1.3 M columns per symbolic tile and 38 K per numeric tile at 160 KB of LDS.  Nothing of
 * it lives in global memory, so there is no workspace limit to respect.  The walks of a hub row grow
 * with the column count (about 400 at 16 M columns) and have been measured up to 4 tiles only;
 * splitting a hub row's products over several workgroups, each with its own tiles, is the way out.
 *
 * Work is split inside a row by TEAMS: team t of a group takes the entries t, t + teams, ... of the
 * row of A and its lanes stride the row of B (8 lanes of 8; 4 teams of 16; 8 teams of 32).
 */
#pragma once

#include <gunrock/hip/primitives.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int SG_BLOCK = 256;
constexpr int SG_SMALL = 8;            // lanes of a sub-wave group
constexpr int SG_SMALL_SLOTS = 64;     // ... and the slots of its table
constexpr int SG_SMALL_PRODUCTS = 32;  // rows of at most this many products may go there
constexpr int SG_WAVE_SLOTS = 512;     // table of a wavefront's row
constexpr int SG_WAVE = 256;           // ... which holds at most this many entries
constexpr int SG_MEDIUM = 2048;        // entries of a medium workgroup row (4096 slots)
constexpr int SG_MIN_SLOTS = 64;       // smallest table of the workgroup path
constexpr int SG_CLASSES = 6;          // empty, sub-wave, wavefront, medium, large, dense
constexpr int SG_EMPTY = -1;

/// Size class of a row of `size` entries (a bound or the exact number) and `products` products.
/// b[0..2]: the most entries of a wavefront row, a medium row and a large row.
__host__ __device__ __forceinline__ unsigned spgemm_class_of(int32_t size, unsigned long long products,
                                                             const int32_t* b, int32_t small_products) {
  return size == 0 ? 0u
         : products <= (unsigned long long)small_products ? 1u
         : size <= b[0] ? 2u
         : size <= b[1] ? 3u
         : size <= b[2] ? 4u
                        : 5u;
}

/// starts[c] = first position of class c in the class-sorted keys (c = 0 .. SG_CLASSES).
__global__ void spgemm_class_starts_kernel(const unsigned* keys, int32_t n, int32_t* starts) {
  const int c = threadIdx.x;
  if (c > SG_CLASSES)
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

/// products[i] = sum over the entries k of row i of A of the length of row k of B; bound[i] =
/// min(products[i], n_cols); totals[0] += the products of all rows.  A wavefront per row.
__global__ void __launch_bounds__(SG_BLOCK)
    spgemm_bound_kernel(const int32_t* ap, const int32_t* aj, const int32_t* bp, int32_t n, int32_t n_cols,
                        unsigned long long* products, int32_t* bound, unsigned long long* totals) {
  constexpr int WAVES = SG_BLOCK / wave_size;
  const int lane = lane_id();
  const int64_t stride = (int64_t)gridDim.x * WAVES;
  unsigned long long all = 0;
  for (int64_t i = (int64_t)blockIdx.x * WAVES + threadIdx.x / wave_size; i < n; i += stride) {
    const int32_t lo = ap[i], hi = ap[i + 1];
    unsigned long long u = 0;
    for (int32_t e = lo + lane; e < hi; e += wave_size) {
      const int32_t k = aj[e];
      u += (unsigned long long)(bp[k + 1] - bp[k]);
    }
    u = wave_sum(u);
    if (lane == 0) {
      products[i] = u;
      bound[i] = (int32_t)(u < (unsigned long long)n_cols ? u : (unsigned long long)n_cols);
      all += u;
    }
  }
  if (lane == 0 && all)
    atomicAdd(&totals[0], all);
}

/// totals[1] += the counts, totals[2] += the rows with a count.
__global__ void __launch_bounds__(SG_BLOCK)
    spgemm_sum_kernel(const int32_t* count, int32_t n, unsigned long long* totals) {
  unsigned long long sum = 0, rows = 0;
  for (int64_t i = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SG_BLOCK) {
    const int32_t c = count[i];
    sum += (unsigned long long)c;
    rows += c > 0;
  }
  sum = wave_sum(sum);
  rows = wave_sum(rows);
  if (lane_id() == 0) {
    if (sum)
      atomicAdd(&totals[1], sum);
    if (rows)
      atomicAdd(&totals[2], rows);
  }
}

/// A relaxed workgroup-scope load of an LDS word that other lanes change with atomics.
template <typename T>
__device__ __forceinline__ T spgemm_peek(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

/// Slot of `col` in the table key[0, mask + 1) (a power of two of slots, fewer than half of them
/// taken by other columns); `fresh` += 1 when this call took the slot.  The probe count is bounded
/// by the table, so a table somebody sized wrongly ends the loop instead of spinning.
__device__ __forceinline__ unsigned spgemm_insert(int32_t* key, unsigned mask, int32_t col, int& fresh) {
  unsigned h = ((unsigned)col * 0x9e3779b1u) >> 7;
  for (unsigned probe = 0; probe <= mask; ++probe, ++h) {
    h &= mask;
    const int32_t seen = spgemm_peek(&key[h]);
    if (seen == col)
      return h;
    if (seen != SG_EMPTY)
      continue;
    const int32_t old = atomicCAS(&key[h], SG_EMPTY, col);
    if (old == SG_EMPTY) {
      ++fresh;
      return h;
    }
    if (old == col)
      return h;
  }
  return h & mask;
}

/// The products of A's entries [lo, hi) over `teams` teams of T lanes: entry lo + team, + teams, ...
/// by team `team`, whose lane `tl` strides the row of B.  body(A's value or 0, position in B).
template <int T, typename body_t>
__device__ __forceinline__ void spgemm_walk(const int32_t* aj, const float* ax, const int32_t* bp, int32_t lo,
                                            int32_t hi, int team, int teams, int tl, bool values, body_t&& body) {
  for (int32_t e = lo + team; e < hi; e += teams) {
    const int32_t k = aj[e];
    const float a = values ? ax[e] : 0.0f;
    const int32_t b1 = bp[k + 1];
    for (int32_t f = bp[k] + tl; f < b1; f += T)
      body(a, f);
  }
}

/// One bitonic pass (k, j) over key/val[0, cap) by `threads` threads, of which this is `t`.
__device__ __forceinline__ void spgemm_bitonic_pass(unsigned* key, float* val, int32_t cap, int32_t k, int32_t j,
                                                    int t, int threads) {
  for (int32_t x = t; x < cap / 2; x += threads) {
    const int32_t i = ((x & ~(j - 1)) << 1) | (x & (j - 1));
    const int32_t p = i | j;
    const unsigned a = key[i], b = key[p];
    if ((a > b) == ((i & k) == 0)) {
      key[i] = b;
      key[p] = a;
      const float va = val[i];
      val[i] = val[p];
      val[p] = va;
    }
  }
}

/**
 * @brief Rows with a table per group of G lanes in static LDS: G = 8 (rows of at most
 * SG_SMALL_PRODUCTS products) or 64 (rows of at most SG_WAVE entries).  !NUMERIC: count[i] = the
 * distinct columns of row i.  NUMERIC: row i of C at cp[i].  Every group of a workgroup runs the same
 * number of batches and the same sort network: the barriers are uniform.
 */
template <int G, bool NUMERIC>
__global__ void __launch_bounds__(SG_BLOCK)
    spgemm_group_kernel(const int32_t* ap, const int32_t* aj, const float* ax, const int32_t* bp, const int32_t* bj,
                        const float* bx, const int32_t* rows, int32_t n_rows, int32_t* count, const int32_t* cp,
                        int32_t* cj, float* cx) {
  static_assert(G == SG_SMALL || G == wave_size, "a group is 8 lanes or a wavefront");
  constexpr int SLOTS = G == SG_SMALL ? SG_SMALL_SLOTS : SG_WAVE_SLOTS;
  constexpr int GROUPS = SG_BLOCK / G;
  constexpr int T = G == SG_SMALL ? 8 : 16;
  __shared__ int32_t s_key[GROUPS * SLOTS];
  __shared__ float s_val[NUMERIC ? GROUPS * SLOTS : 1];
  const int l = threadIdx.x % G;
  const int group = threadIdx.x / G;
  int32_t* key = s_key + group * SLOTS;
  float* val = s_val + (NUMERIC ? group * SLOTS : 0);
  for (int64_t r0 = (int64_t)blockIdx.x * GROUPS; r0 < n_rows; r0 += (int64_t)gridDim.x * GROUPS) {
    const int64_t r = r0 + group;
    int32_t i = -1, lo = 0, hi = 0;
    if (r < n_rows) {
      i = rows[r];
      lo = ap[i];
      hi = ap[i + 1];
    }
    for (int s = l; s < SLOTS; s += G) {
      key[s] = SG_EMPTY;
      if (NUMERIC)
        val[s] = 0.0f;
    }
    __syncthreads();
    int fresh = 0;
    spgemm_walk<T>(aj, ax, bp, lo, hi, l / T, G / T, l % T, NUMERIC, [&](float a, int32_t f) {
      const unsigned slot = spgemm_insert(key, SLOTS - 1, bj[f], fresh);
      if (NUMERIC)
        atomicAdd(&val[slot], a * bx[f]);
    });
    __syncthreads();
    if (!NUMERIC) {
#pragma unroll
      for (int d = G / 2; d > 0; d >>= 1)
        fresh += __shfl_xor(fresh, d, G);
      if (l == 0 && i >= 0)
        count[i] = fresh;
    } else {
      for (int32_t k = 2; k <= SLOTS; k <<= 1)
        for (int32_t j = k >> 1; j > 0; j >>= 1) {
          spgemm_bitonic_pass(reinterpret_cast<unsigned*>(key), val, SLOTS, k, j, l, G);
          __syncthreads();
        }
      if (i >= 0) {
        const int32_t at = cp[i];
        const int32_t d = min(cp[i + 1] - at, SLOTS);
        for (int32_t s = l; s < d; s += G) {
          cj[at + s] = key[s];
          cx[at + s] = val[s];
        }
      }
      __syncthreads();  // the next batch clears the table
    }
  }
}

/**
 * @brief One workgroup per row, the table in dynamic LDS: keys at [0, max_slots), values behind
 * them when NUMERIC.  size[i]: the bound (!NUMERIC) or the exact entries (NUMERIC) of row i, at most
 * max_slots / 2; the row's table is the power of two >= 2 * size[i], at least SG_MIN_SLOTS.
 */
template <bool NUMERIC>
__global__ void __launch_bounds__(SG_BLOCK)
    spgemm_block_kernel(const int32_t* ap, const int32_t* aj, const float* ax, const int32_t* bp, const int32_t* bj,
                        const float* bx, const int32_t* rows, int32_t n_rows, const int32_t* size, int32_t max_slots,
                        int32_t* count, const int32_t* cp, int32_t* cj, float* cx) {
  extern __shared__ int32_t s_dyn[];
  __shared__ int s_wave[SG_BLOCK / wave_size];
  constexpr int T = 32;
  const int tid = threadIdx.x;
  int32_t* key = s_dyn;
  float* val = reinterpret_cast<float*>(s_dyn + (NUMERIC ? max_slots : 0));
  for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const int32_t i = rows[r];
    const int32_t lo = ap[i], hi = ap[i + 1];
    const int32_t need = NUMERIC ? cp[i + 1] - cp[i] : size[i];
    int32_t cap = SG_MIN_SLOTS;
    while (cap < max_slots && cap < 2 * (int64_t)need)
      cap <<= 1;
    for (int32_t s = tid; s < cap; s += SG_BLOCK) {
      key[s] = SG_EMPTY;
      if (NUMERIC)
        val[s] = 0.0f;
    }
    __syncthreads();
    int fresh = 0;
    spgemm_walk<T>(aj, ax, bp, lo, hi, tid / T, SG_BLOCK / T, tid % T, NUMERIC, [&](float a, int32_t f) {
      const unsigned slot = spgemm_insert(key, (unsigned)cap - 1, bj[f], fresh);
      if (NUMERIC)
        atomicAdd(&val[slot], a * bx[f]);
    });
    if (!NUMERIC) {
      const int total = block_sum<SG_BLOCK>(fresh, s_wave);
      if (tid == 0)
        count[i] = total;
      __syncthreads();  // s_wave and the table are the next row's
    } else {
      __syncthreads();
      for (int32_t k = 2; k <= cap; k <<= 1)
        for (int32_t j = k >> 1; j > 0; j >>= 1) {
          spgemm_bitonic_pass(reinterpret_cast<unsigned*>(key), val, cap, k, j, tid, SG_BLOCK);
          __syncthreads();
        }
      const int32_t at = cp[i];
      const int32_t d = min(need, cap);
      for (int32_t s = tid; s < d; s += SG_BLOCK) {
        cj[at + s] = key[s];
        cx[at + s] = val[s];
      }
      __syncthreads();
    }
  }
}

/**
 * @brief One workgroup per row, a tile of `tile` columns (a multiple of 32) at a time in dynamic
 * LDS: tile / 32 bitmap words, then `tile` floats when NUMERIC.  Each tile walks all products of the
 * row and keeps those whose column it holds; the bitmap read in order gives the tile's part of the
 * row, sorted.  !NUMERIC: count[i].  NUMERIC: row i of C at cp[i], never past cp[i + 1].
 */
template <bool NUMERIC>
__global__ void __launch_bounds__(SG_BLOCK)
    spgemm_dense_kernel(const int32_t* ap, const int32_t* aj, const float* ax, const int32_t* bp, const int32_t* bj,
                        const float* bx, const int32_t* rows, int32_t n_rows, int32_t n_cols, int32_t tile,
                        int32_t* count, const int32_t* cp, int32_t* cj, float* cx) {
  extern __shared__ int32_t s_dyn[];
  __shared__ int32_t s_wave[SG_BLOCK / wave_size + 1];
  constexpr int T = 32;
  const int tid = threadIdx.x;
  unsigned* bits = reinterpret_cast<unsigned*>(s_dyn);
  float* val = reinterpret_cast<float*>(s_dyn + tile / 32);
  for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const int32_t i = rows[r];
    const int32_t lo = ap[i], hi = ap[i + 1];
    int32_t out = NUMERIC ? cp[i] : 0;
    const int32_t end = NUMERIC ? cp[i + 1] : 0;
    int32_t mine = 0;
    for (int64_t c0 = 0; c0 < n_cols; c0 += tile) {
      const int32_t w = (int32_t)min((int64_t)tile, (int64_t)n_cols - c0);
      const int32_t words = (w + 31) / 32;
      for (int32_t s = tid; s < words; s += SG_BLOCK)
        bits[s] = 0u;
      if (NUMERIC)
        for (int32_t s = tid; s < w; s += SG_BLOCK)
          val[s] = 0.0f;
      __syncthreads();
      spgemm_walk<T>(aj, ax, bp, lo, hi, tid / T, SG_BLOCK / T, tid % T, NUMERIC, [&](float a, int32_t f) {
        const int64_t c = (int64_t)bj[f] - c0;
        if (c >= 0 && c < w) {
          const unsigned bit = 1u << (c & 31);
          if (!(spgemm_peek(&bits[c >> 5]) & bit))
            atomicOr(&bits[c >> 5], bit);
          if (NUMERIC)
            atomicAdd(&val[c], a * bx[f]);
        }
      });
      __syncthreads();
      // each thread a contiguous run of bitmap words
      const int32_t per = (words + SG_BLOCK - 1) / SG_BLOCK;
      const int32_t w0 = min(words, tid * per), w1 = min(words, w0 + per);
      int32_t cnt = 0;
      for (int32_t s = w0; s < w1; ++s)
        cnt += __popc(bits[s]);
      if (!NUMERIC) {
        mine += cnt;
      } else {
        int32_t P = 0;
        int32_t pos = out + block_exclusive_sum<SG_BLOCK>(cnt, P, s_wave);
        for (int32_t s = w0; s < w1; ++s)
          for (unsigned m = bits[s]; m; m &= m - 1) {
            const int32_t c = s * 32 + (__ffs(m) - 1);
            if (pos < end) {
              cj[pos] = (int32_t)(c0 + c);
              cx[pos] = val[c];
            }
            ++pos;
          }
        out += P;
      }
      __syncthreads();  // the next tile clears what was just read
    }
    if (!NUMERIC) {
      const int32_t total = block_sum<SG_BLOCK>(mine, s_wave);
      if (tid == 0)
        count[i] = total;
      __syncthreads();
    }
  }
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

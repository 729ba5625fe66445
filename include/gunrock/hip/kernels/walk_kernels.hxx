/**
 * @file walk_kernels.hxx
 * @brief Random walks (grx_random_walk, include/essentials_amd.h): first-order uniform and weighted
 * walks and node2vec by rejection, every draw a function of (seed, walk, step, draw index) alone.
 *
 * The first half of the file is the DEFINITION of a step and compiles as plain C++
 * (tests/cpp/walk_pick_tests.cpp): the counter-based draws and the three selection functions --
 * uniform index, weighted search in the prefix array with its `== W` fallback, and the ratio class
 * of a node2vec candidate.  The kernels below call exactly these.
 *
 * Kernels: the prefix array of a weighted call (4 bytes per entry, built in the order the header
 * fixes: sequential inside blocks of 64 entries, block bases added sequentially per row), and the
 * walker, one lane per walk.  A step is a chain of dependent random loads (the offset pair, then
 * the column entry, then log d prefix probes when weighted): nothing in it is wide, so rows of every
 * length take the same path and the only lever is the number of walks in flight.
 */
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GRX_WALK_HD __host__ __device__
#else
#define GRX_WALK_HD
#endif

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int WALK_PREFIX_BLOCK = 64;     // entries per prefix block: part of the definition
constexpr int WALK_MAX_ATTEMPTS = 1024;   // node2vec: candidates per step, default and maximum
constexpr int WALK_LEVELS = 64;           // grx_stats::frontier_slots

enum walk_ratio_t : int { WALK_RET = 0, WALK_ADJ = 1, WALK_FAR = 2 };

/// rmat.hip's mix64: the splitmix64 finaliser of x + 0x9E3779B97F4A7C15.
GRX_WALK_HD inline unsigned long long walk_mix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

/// What the draws of walk `i` share: r(i, t, j) = walk_draw(walk_stream(seed, i), t, j).
GRX_WALK_HD inline unsigned long long walk_stream(unsigned long long seed, unsigned long long i) {
  return walk_mix64(seed ^ walk_mix64(i));
}
GRX_WALK_HD inline unsigned long long walk_draw(unsigned long long stream, unsigned t, unsigned long long j) {
  return walk_mix64(stream + ((unsigned long long)t << 32) + j);
}

/// The top 24 bits as a float in [0, 1): exact.
GRX_WALK_HD inline float walk_u24(unsigned long long r) { return (float)(r >> 40) * 0x1p-24f; }

/// Uniform candidate of a row of `d` entries: the top 32 bits of r scaled to [0, d) in 64-bit integers.
GRX_WALK_HD inline long long walk_pick_uniform(unsigned long long r, long long d) {
  return (long long)(((r >> 32) * (unsigned long long)d) >> 32);
}

/// Weighted candidate of a row whose prefix array is c[0, d), d >= 1, W = c[d - 1]: the smallest k
/// with c[k] > fl(u24(r) * W); when the product rounded up to W, the smallest k with c[k] == W.
/// Never outside [0, d), whatever the weights are.
GRX_WALK_HD inline long long walk_pick_weighted(const float* c, long long d, unsigned long long r) {
  const float W = c[d - 1];
  const float x = walk_u24(r) * W;
  long long lo = 0, hi = d;  // c[k] <= x for k < lo, c[k] > x for k >= hi
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (c[mid] > x)
      hi = mid;
    else
      lo = mid + 1;
  }
  if (lo < d)
    return lo;
  lo = 0, hi = d - 1;  // c[d - 1] == W
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (c[mid] >= W)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

/// The class of candidate x of a step that came from `prev`: back to it, to one of its own
/// neighbours (the entry prev -> x exists: `prev_row` is row prev SORTED by column, `len` entries),
/// or further away.
GRX_WALK_HD inline int walk_ratio_class(int32_t x, int32_t prev, const int32_t* prev_row, long long len) {
  if (x == prev)
    return WALK_RET;
  long long lo = 0, hi = len;
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (prev_row[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < len && prev_row[lo] == x ? WALK_ADJ : WALK_FAR;
}

// A translation unit that wants the definition alone (the draws, for another sampler) says so: the
// kernels below are not templates, and one library holds them once.
#if defined(__HIPCC__) && !defined(GRX_WALK_DEFINITION_ONLY)

constexpr int WALK_BLOCK = 256;
constexpr int WALK_PREFIX_THREADS = 128;  // two wavefronts, a 64 x 65 float tile each
constexpr int WALK_TILE_STRIDE = WALK_PREFIX_BLOCK + 1;

/// Device counters of a call, unsigned long long each.
enum walk_counter_t : int {
  WC_TOOK = 0,                      // [n], n = 0..64: walks that took min(n, 64) steps
  WC_STEPS = WALK_LEVELS + 1,       // steps taken
  WC_ATTEMPTS,                      // candidates drawn
  WC_LONGEST,                       // the largest number of steps of a walk
  WC_FULL,                          // walks that took all `length` steps
  WC_COUNT
};

/// Prefix blocks of a row of d entries.
__host__ __device__ inline int32_t walk_blocks_of(int32_t d) { return (d + WALK_PREFIX_BLOCK - 1) / WALK_PREFIX_BLOCK; }

/// Where prefix block B lies: first_block[0, n] is the exclusive sum of walk_blocks_of over the rows.
struct walk_block_t {
  int32_t start;  // its first entry
  int32_t len;    // 1..64 entries; 0: no such block
  int32_t index;  // its place in its row
};
__device__ inline walk_block_t walk_locate(const int32_t* ap, const int32_t* first_block, int32_t n, int32_t B,
                                           int32_t n_blocks) {
  if (B >= n_blocks)
    return {0, 0, 0};
  int32_t lo = 0, hi = n;  // first_block[lo] <= B < first_block[hi]; the last such lo is the row with blocks
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (first_block[mid] <= B)
      lo = mid;
    else
      hi = mid;
  }
  const int32_t b = B - first_block[lo];
  const int32_t start = ap[lo] + b * WALK_PREFIX_BLOCK;  // < nnz <= INT32_MAX
  const int32_t left = ap[lo + 1] - start;
  return {start, left < WALK_PREFIX_BLOCK ? left : WALK_PREFIX_BLOCK, b};
}

/// c[e] = the sequential float32 sum of the weights of e's block up to e, and last[B] = the sum of
/// block B.  A wavefront takes 64 consecutive blocks: their entries are read and written a block at
/// a time by all lanes, and lane l sums block l in a padded LDS tile.
__global__ void __launch_bounds__(WALK_PREFIX_THREADS)
    walk_prefix_local_kernel(const int32_t* ap, const float* ax, const int32_t* first_block, int32_t n,
                             int32_t n_blocks, float* c, float* last) {
  __shared__ float s_tile[WALK_PREFIX_THREADS / 64][WALK_PREFIX_BLOCK * WALK_TILE_STRIDE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* tile = s_tile[wave];
  const long long B0 = ((long long)blockIdx.x * (WALK_PREFIX_THREADS / 64) + wave) * 64;
  const int32_t B = (int32_t)(B0 + lane < n_blocks ? B0 + lane : n_blocks);
  const walk_block_t mine = walk_locate(ap, first_block, n, B, n_blocks);
  for (int j = 0; j < 64; ++j) {
    const int32_t start = __shfl(mine.start, j, 64), len = __shfl(mine.len, j, 64);
    if (lane < len)
      tile[j * WALK_TILE_STRIDE + lane] = ax[(long long)start + lane];
  }
  __syncthreads();
  if (mine.len) {
    float* row = tile + lane * WALK_TILE_STRIDE;
    float sum = row[0];
    for (int k = 1; k < mine.len; ++k) {
      sum = sum + row[k];
      row[k] = sum;
    }
    last[B] = sum;
  }
  __syncthreads();
  for (int j = 0; j < 64; ++j) {
    const int32_t start = __shfl(mine.start, j, 64), len = __shfl(mine.len, j, 64);
    if (lane < len)
      c[(long long)start + lane] = tile[j * WALK_TILE_STRIDE + lane];
  }
}

/// Per row of more than one block: last[B] becomes the base of block B, B_0 = 0 and
/// B_{b+1} = fl(B_b + the sum of block b), in block order.
__global__ void __launch_bounds__(WALK_BLOCK)
    walk_prefix_base_kernel(const int32_t* first_block, int32_t n, float* last) {
  for (long long v = blockIdx.x * (long long)WALK_BLOCK + threadIdx.x; v < n; v += (long long)gridDim.x * WALK_BLOCK) {
    const int32_t begin = first_block[v], end = first_block[v + 1];
    if (end - begin < 2)
      continue;
    float base = 0.0f;
    for (int32_t B = begin; B < end; ++B) {
      const float sum = last[B];
      last[B] = base;
      base = base + sum;
    }
  }
}

/// c[e] = fl(base of e's block + c[e]) for the blocks behind the first of their row.
__global__ void __launch_bounds__(WALK_BLOCK)
    walk_prefix_apply_kernel(const int32_t* ap, const int32_t* first_block, int32_t n, int32_t n_blocks,
                             const float* base, float* c) {
  const int lane = threadIdx.x & 63;
  const long long B0 = ((long long)blockIdx.x * (WALK_BLOCK / 64) + (threadIdx.x >> 6)) * 64;
  const int32_t B = (int32_t)(B0 + lane < n_blocks ? B0 + lane : n_blocks);
  const walk_block_t mine = walk_locate(ap, first_block, n, B, n_blocks);
  const float my_base = mine.len && mine.index ? base[B] : 0.0f;
  for (int j = 0; j < 64; ++j) {
    const int32_t start = __shfl(mine.start, j, 64), len = __shfl(mine.len, j, 64);
    const int32_t index = __shfl(mine.index, j, 64);
    const float b = __shfl(my_base, j, 64);
    if (index && lane < len)
      c[(long long)start + lane] = b + c[(long long)start + lane];
  }
}

struct walk_args_t {
  const int32_t* ap;
  const int32_t* aj;
  const float* c;          // the prefix array (weighted walks)
  const int32_t* sorted;   // the columns of every row in ascending order (second-order walks)
  const int32_t* starts;   // nullptr: walk i starts at vertex i
  long long count;
  int32_t length;
  unsigned long long seed;
  float ret, adj, far;     // acceptance ratios by walk_ratio_t
  int32_t cap;             // candidates per step
  int32_t* walks;
  unsigned long long* counters;
};

constexpr int WALK_STAGE = 16;  // steps of a walk that leave the wavefront as one 64-byte piece

/// One lane per walk.  WEIGHTED: candidates by the prefix array; SECOND: node2vec's rejection test
/// from step 2 on.  A lane's vertices go to its row of an LDS tile and leave every WALK_STAGE steps:
/// four walks per store instruction, sixteen consecutive slots each, so a walk's row is written in
/// 64-byte pieces instead of one 4-byte store per lane and step.  Every lane of the workgroup runs
/// all `length` steps of the loop, a finished or absent walk as a -1 that is (not) written.
template <bool WEIGHTED, bool SECOND>
__global__ void __launch_bounds__(WALK_BLOCK) walk_kernel(const walk_args_t a) {
  __shared__ unsigned long long s_counters[WC_COUNT];
  __shared__ int32_t s_stage[WALK_BLOCK / 64][64][WALK_STAGE + 1];
  for (int k = threadIdx.x; k < WC_COUNT; k += WALK_BLOCK)
    s_counters[k] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  int32_t(*stage)[WALK_STAGE + 1] = s_stage[threadIdx.x >> 6];
  const long long i = blockIdx.x * (long long)WALK_BLOCK + threadIdx.x;
  const long long first = i - lane, width = (long long)a.length + 1;
  const bool mine = i < a.count;
  bool walking = mine;
  int32_t v = !mine ? -1 : a.starts ? a.starts[i] : (int32_t)i;
  const unsigned long long stream = walk_stream(a.seed, (unsigned long long)i);
  int32_t prev_lo = 0, prev_hi = 0, prev = -1;
  int32_t steps = 0;
  unsigned long long attempts = 0;
  for (int32_t t = 0; t <= a.length; ++t) {
    if (t > 0 && walking) {
      const int32_t lo = a.ap[v], hi = a.ap[v + 1];
      const int32_t d = hi - lo;
      if (d == 0 || (WEIGHTED && !(a.c[hi - 1] > 0.0f))) {
        walking = false;
        v = -1;
      } else {
        int32_t x, tried = 0;
        for (;;) {
          const unsigned long long r = walk_draw(stream, (unsigned)t, 2ull * (unsigned)tried);
          const long long k = WEIGHTED ? walk_pick_weighted(a.c + lo, d, r) : walk_pick_uniform(r, d);
          x = a.aj[lo + k];
          ++tried;
          if (!SECOND || t == 1)
            break;
          const int cls = walk_ratio_class(x, prev, a.sorted + prev_lo, prev_hi - prev_lo);
          const float ratio = cls == WALK_RET ? a.ret : cls == WALK_ADJ ? a.adj : a.far;
          if (ratio == 1.0f || tried >= a.cap)
            break;
          if (walk_u24(walk_draw(stream, (unsigned)t, 2ull * (unsigned)(tried - 1) + 1)) < ratio)
            break;
        }
        attempts += (unsigned long long)tried;
        prev = v;
        prev_lo = lo;
        prev_hi = hi;
        v = x;
        ++steps;
      }
    }
    const int slot = t & (WALK_STAGE - 1);
    stage[lane][slot] = v;
    if (slot == WALK_STAGE - 1 || t == a.length) {  // the same t in every lane: the wavefront is whole here
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int s = lane & (WALK_STAGE - 1);
      for (int j = lane / WALK_STAGE; j < 64; j += 64 / WALK_STAGE) {
        const long long walk = first + j;
        if (s <= slot && walk < a.count)
          a.walks[walk * width + (t - slot) + s] = stage[j][s];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  if (mine) {
    atomicAdd(&s_counters[WC_TOOK + (steps < WALK_LEVELS ? steps : WALK_LEVELS)], 1ull);
    atomicAdd(&s_counters[WC_STEPS], (unsigned long long)steps);
    atomicAdd(&s_counters[WC_ATTEMPTS], attempts);
    atomicMax(&s_counters[WC_LONGEST], (unsigned long long)steps);
    if (steps == a.length)
      atomicAdd(&s_counters[WC_FULL], 1ull);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < WC_COUNT; k += WALK_BLOCK)
    if (const unsigned long long x = s_counters[k]) {
      if (k == WC_LONGEST)
        atomicMax(&a.counters[k], x);
      else
        atomicAdd(&a.counters[k], x);
    }
}

#endif  // __HIPCC__

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

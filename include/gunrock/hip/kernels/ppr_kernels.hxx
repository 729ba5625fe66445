/**
 * @file ppr_kernels.hxx
 * @brief Batched personalized PageRank (grx_ppr): up to 64 seeds share one read of every in-entry
 * through the lanes of a wavefront.  Lane = column (seed) of the batch; an entry (u -> v, w) costs one
 * load of (u, w) and one contiguous L * 4-byte read of give[u].
 *
 * State of a batch, vertex-major with L = 16, 32 or 64 columns (the smallest that holds the batch):
 * p[V][L] and two arrays give[V][L] that take turns, give[u][c] = p[u][c] * scale[u]: what u hands
 * each out-neighbour per unit weight.  A wavefront holds 64 / L lane groups, a group sums one in-row.
 * Columns at or beyond the batch's width are frozen from the start and stay 0.  Invariants between
 * iterations (behind the publish kernel of iteration t):
 *
 *   p holds p_t, the current give array holds p_t * scale, for every vertex and column;
 *   ctr->dangling[c] holds D_t, the sum of p_t[u][c] over the dangling list;
 *   ctr->maxdiff[] is 0; ctr->frozen has bit c set iff column c no longer changes.
 *
 * An iteration is, in launch order:
 *
 *   ppr_gather_kernel    every in-row of at most `segment` entries: the sequential sum in row order
 *                        (ppr_row_sum, PPR_FLIGHT row reads in flight), then ppr_finish: the seed
 *                        term in the lane whose seed is v, |new - old|, p and the next give.  A frozen
 *                        lane copies its give word and leaves p alone.
 *   ppr_segment_kernel   the longer in-rows were cut once per call into items {v, k} of `segment`
 *                        entries (ppr_items_kernel); a lane group sums one item into partial[item].
 *   ppr_combine_kernel   a lane group per long row adds its partials in segment order, ppr_finish.
 *   ppr_dangling_kernel  a lane group per PPR_DANGLING_CHUNK entries of the ascending dangling list
 *                        sums p_t[u] sequentially into dpart[chunk].
 *   ppr_publish_kernel   one wavefront, lane = column: adds dpart in chunk order into ctr->dangling,
 *                        folds maxdiff into iterations / residual, freezes the columns below tol,
 *                        clears maxdiff, hands the frozen mask to the host and stamps.
 *
 * Every float sum above has an order fixed by the in-row layout, V, `segment` and the two constants;
 * none depends on the grid.  The per-column largest difference goes through LDS and one atomicMax on
 * the float's bits per workgroup and column: non-negative floats order like unsigned integers and a
 * maximum does not depend on the order.  Products and sums are spelled with __fmaf_rn / __fadd_rn /
 * __fmul_rn so that every width L and every kernel rounds alike.  No kernel waits on another
 * workgroup.  ppr_deliver_kernel transposes p through LDS into the caller's rows.
 */
#pragma once

#include <gunrock/hip/kernels/group_rows.hxx>  // csr_rows_t, here the in-entries

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int PPR_BLOCK = 256;
constexpr int PPR_BATCH = 64;              // seeds per batch: the lanes of a wavefront
constexpr int PPR_SEGMENT = 512;           // default: in-row entries one lane group sums
constexpr int PPR_SEGMENT_MIN = 64;
constexpr int PPR_FLIGHT = 8;              // row reads in flight per lane group
constexpr int PPR_DANGLING_CHUNK = 1024;   // dangling vertices per first-stage sum
constexpr int PPR_TILE = 64;               // vertices per delivery tile

/// Device state of one batch.
struct ppr_counters_t {
  unsigned maxdiff[PPR_BATCH];             // bits of the largest |new - old| of the running iteration
  unsigned long long nonzero[PPR_BATCH];   // delivered values > 0
  int iterations[PPR_BATCH];
  float residual[PPR_BATCH];
  float dangling[PPR_BATCH];               // D_t of the p the state holds
  unsigned long long frozen;
};
enum { PM_FROZEN = 0, PM_WORDS };

/// The seeds of a batch, by value; -1 in a column the batch does not use.
struct ppr_seeds_t {
  int32_t v[PPR_BATCH];
};

/// What the kernels that finish a vertex share.
struct ppr_state_t {
  const float* scale;
  float* p;
  const float* give;   // p_t * scale
  float* next;         // p_{t+1} * scale
  ppr_seeds_t seeds;
  unsigned long long frozen;
  float alpha;
  ppr_counters_t* ctr;
};

template <int L>
struct ppr_shape_t {
  static constexpr int groups = PPR_BLOCK / L;  // in-rows a workgroup sums side by side
};

/// The lane's row of the workgroup and its column.
template <int L>
__device__ __forceinline__ void ppr_place(int& group, int& column) {
  group = (int)threadIdx.x / L;
  column = (int)threadIdx.x % L;
  if (L == wave_size)  // the whole wavefront is on one row: its offsets and entries are scalar
    group = __builtin_amdgcn_readfirstlane(group);
}

/// Sum over entries [lo, hi) of give[source][c] * weight, sequentially in entry order from 0.
template <int L>
__device__ __forceinline__ float ppr_row_sum(const csr_rows_t& in, const float* give, int32_t lo, int32_t hi, int c) {
  float acc = 0.0f;
  int32_t e = lo;
  if (e + PPR_FLIGHT <= hi) {
    int32_t u[PPR_FLIGHT], u_next[PPR_FLIGHT];
    float w[PPR_FLIGHT], w_next[PPR_FLIGHT], x[PPR_FLIGHT];
#pragma unroll
    for (int k = 0; k < PPR_FLIGHT; ++k) {
      u[k] = in.aj[e + k];
      w[k] = in.ax[e + k];
    }
    for (;;) {
#pragma unroll
      for (int k = 0; k < PPR_FLIGHT; ++k)
        x[k] = give[(std::size_t)u[k] * L + c];
      e += PPR_FLIGHT;
      const bool more = e + PPR_FLIGHT <= hi;
      if (more) {  // the next entries come in behind this group's row reads
#pragma unroll
        for (int k = 0; k < PPR_FLIGHT; ++k) {
          u_next[k] = in.aj[e + k];
          w_next[k] = in.ax[e + k];
        }
      }
#pragma unroll
      for (int k = 0; k < PPR_FLIGHT; ++k)
        acc = __fmaf_rn(x[k], w[k], acc);
      if (!more)
        break;
#pragma unroll
      for (int k = 0; k < PPR_FLIGHT; ++k) {
        u[k] = u_next[k];
        w[k] = w_next[k];
      }
    }
  }
  if (e < hi) {  // the last entries, fewer than PPR_FLIGHT: read together (a slot past the end rereads
                 // the last entry), added in order
    int32_t u[PPR_FLIGHT];
    float w[PPR_FLIGHT], x[PPR_FLIGHT];
#pragma unroll
    for (int k = 0; k < PPR_FLIGHT; ++k) {
      const int32_t at = min(e + k, hi - 1);
      u[k] = in.aj[at];
      w[k] = in.ax[at];
    }
#pragma unroll
    for (int k = 0; k < PPR_FLIGHT; ++k)
      x[k] = give[(std::size_t)u[k] * L + c];
#pragma unroll
    for (int k = 0; k < PPR_FLIGHT; ++k)
      if (e + k < hi)
        acc = __fmaf_rn(x[k], w[k], acc);
  }
  return acc;
}

/// The lane's seed term of this iteration: (1 - alpha) + alpha * D_t.
__device__ __forceinline__ float ppr_seed_term(const ppr_state_t& s, int c) {
  return __fmaf_rn(s.alpha, s.ctr->dangling[c], 1.0f - s.alpha);
}

/// acc is the sum over v's in-entries for column c: write p and the next give; returns |new - old|.
template <int L>
__device__ __forceinline__ float ppr_finish(const ppr_state_t& s, int32_t v, int c, int32_t seed, float seed_term,
                                            float acc) {
  const std::size_t at = (std::size_t)v * L + c;
  if ((s.frozen >> c) & 1) {  // the column keeps its values: the next give is the old one
    s.next[at] = s.give[at];
    return 0.0f;
  }
  const float now = v == seed ? __fadd_rn(acc, seed_term) : acc;
  const float old = s.p[at];
  s.p[at] = now;
  s.next[at] = __fmul_rn(now, s.scale[v]);
  return fabsf(now - old);
}

/// Ends a finishing kernel: the workgroup's largest difference per column, one atomic each.  Every
/// thread of the workgroup calls it.  `s_diff`: PPR_BATCH words of LDS, zeroed behind a barrier.
template <int L>
__device__ __forceinline__ void ppr_flush(float worst, int c, unsigned* s_diff, ppr_counters_t* ctr) {
  if (worst > 0.0f)
    atomicMax(&s_diff[c], __float_as_uint(worst));
  __syncthreads();
  if ((int)threadIdx.x < L) {
    const unsigned d = s_diff[threadIdx.x];
    if (d)
      atomicMax(&ctr->maxdiff[threadIdx.x], d);
  }
}

/// Once per call: scale[u] = alpha / W(u), W(u) the sum of row u's weights (0 when that sum is 0),
/// and the two flags the lists are built from.  A wavefront per row: lane l sums entries l, l + 64,
/// ... in order, the 64 sums meet in a butterfly -- an order fixed by the row alone.
__global__ void __launch_bounds__(PPR_BLOCK)
    ppr_scale_kernel(const int32_t* ap, const float* ax, csr_rows_t in, float alpha, int32_t n, int32_t segment,
                     float* scale, unsigned char* is_dangling, unsigned char* is_long) {
  const int lane = lane_id();
  const int64_t waves = (int64_t)gridDim.x * (PPR_BLOCK / wave_size);
  for (int64_t v = (int64_t)blockIdx.x * (PPR_BLOCK / wave_size) + threadIdx.x / wave_size; v < n; v += waves) {
    const int32_t lo = ap[v], hi = ap[v + 1];
    float w = 0.0f;
    for (int32_t e = lo + lane; e < hi; e += wave_size)
      w = __fadd_rn(w, ax[e]);
    w = wave_sum(w);
    if (lane == 0) {
      scale[v] = w != 0.0f ? alpha / w : 0.0f;
      is_dangling[v] = w != 0.0f ? 0 : 1;
      is_long[v] = in.ap[v + 1] - in.ap[v] > segment ? 1 : 0;
    }
  }
}

/// Once per call, one workgroup: first[r] = the first item of long row r (first[rows] = the items),
/// and the items {vertex, segment} themselves, row after row.
__global__ void __launch_bounds__(PPR_BLOCK)
    ppr_items_kernel(csr_rows_t in, const int32_t* long_rows, const int32_t* n_long, int32_t segment, int32_t* first,
                     int2* items, int32_t capacity) {
  __shared__ int32_t s_wave[PPR_BLOCK / wave_size + 1];
  const int32_t rows = *n_long;
  int32_t base = 0;
  for (int32_t r0 = 0; r0 < rows; r0 += PPR_BLOCK) {
    const int32_t r = r0 + (int32_t)threadIdx.x;
    int32_t v = 0, segments = 0;
    if (r < rows) {
      v = long_rows[r];
      segments = (in.ap[v + 1] - in.ap[v] + segment - 1) / segment;
    }
    int32_t total = 0;
    const int32_t at = base + block_exclusive_sum<PPR_BLOCK>(segments, total, s_wave);
    if (r < rows) {
      first[r] = at;
      for (int32_t k = 0; k < segments; ++k)
        if (at + k < capacity)  // sized by the host from nnz, so this holds; it guards the store all the same
          items[at + k] = make_int2(v, k);
    }
    base += total;
  }
  if (threadIdx.x == 0)
    first[rows] = base;
}

/// A batch begins: p = e_seed per column, give = p * scale, D_0 = [the seed is dangling].  p and the
/// current give array were zeroed before it.  One wavefront.
template <int L>
__global__ void ppr_seed_kernel(ppr_seeds_t seeds, int width, const float* scale, float* p, float* give,
                                ppr_counters_t* ctr, unsigned long long frozen) {
  const int c = threadIdx.x;
  if (c < width) {
    const int32_t s = seeds.v[c];
    const float sc = scale[s];
    p[(std::size_t)s * L + c] = 1.0f;
    give[(std::size_t)s * L + c] = sc;
    ctr->dangling[c] = sc == 0.0f ? 1.0f : 0.0f;
  }
  if (c == 0)
    ctr->frozen = frozen;
}

/// The in-rows of at most `segment` entries, a lane group each.
template <int L>
__global__ void __launch_bounds__(PPR_BLOCK) ppr_gather_kernel(csr_rows_t in, ppr_state_t s, int32_t n, int32_t segment) {
  __shared__ unsigned s_diff[PPR_BATCH];
  if (threadIdx.x < PPR_BATCH)
    s_diff[threadIdx.x] = 0;
  __syncthreads();
  int group, c;
  ppr_place<L>(group, c);
  const int32_t seed = s.seeds.v[c];
  const float seed_term = ppr_seed_term(s, c);
  float worst = 0.0f;
  constexpr int ROWS = ppr_shape_t<L>::groups;
  for (int64_t v0 = (int64_t)blockIdx.x * ROWS; v0 < n; v0 += (int64_t)gridDim.x * ROWS) {
    const int64_t v = v0 + group;
    if (v >= n)
      continue;
    const int32_t lo = in.ap[v], hi = in.ap[v + 1];
    if (hi - lo > segment)  // ppr_combine_kernel finishes it
      continue;
    const float acc = ppr_row_sum<L>(in, s.give, lo, hi, c);
    worst = fmaxf(worst, ppr_finish<L>(s, (int32_t)v, c, seed, seed_term, acc));
  }
  ppr_flush<L>(worst, c, s_diff, s.ctr);
}

/// The items of the long in-rows, a lane group each: partial[item] = the sum over its segment.
template <int L>
__global__ void __launch_bounds__(PPR_BLOCK)
    ppr_segment_kernel(csr_rows_t in, const float* give, const int2* items, int32_t n_items, int32_t segment,
                       float* partial) {
  int group, c;
  ppr_place<L>(group, c);
  constexpr int ROWS = ppr_shape_t<L>::groups;
  for (int64_t i0 = (int64_t)blockIdx.x * ROWS; i0 < n_items; i0 += (int64_t)gridDim.x * ROWS) {
    const int64_t i = i0 + group;
    if (i >= n_items)
      continue;
    const int2 item = items[i];
    const int64_t end = in.ap[item.x + 1];
    const int64_t lo = (int64_t)in.ap[item.x] + (int64_t)item.y * segment;
    const int64_t hi = min(end, lo + segment);
    partial[(std::size_t)i * L + c] = ppr_row_sum<L>(in, give, (int32_t)lo, (int32_t)hi, c);
  }
}

/// The long in-rows, a lane group each: the partials in segment order, then ppr_finish.
template <int L>
__global__ void __launch_bounds__(PPR_BLOCK)
    ppr_combine_kernel(ppr_state_t s, const int32_t* long_rows, const int32_t* first, int32_t n_long,
                       const float* partial) {
  __shared__ unsigned s_diff[PPR_BATCH];
  if (threadIdx.x < PPR_BATCH)
    s_diff[threadIdx.x] = 0;
  __syncthreads();
  int group, c;
  ppr_place<L>(group, c);
  const int32_t seed = s.seeds.v[c];
  const float seed_term = ppr_seed_term(s, c);
  float worst = 0.0f;
  constexpr int ROWS = ppr_shape_t<L>::groups;
  for (int64_t r0 = (int64_t)blockIdx.x * ROWS; r0 < n_long; r0 += (int64_t)gridDim.x * ROWS) {
    const int64_t r = r0 + group;
    if (r >= n_long)
      continue;
    const int32_t a = first[r], b = first[r + 1];
    float acc = 0.0f;
    for (int32_t k = a; k < b; ++k)
      acc = __fadd_rn(acc, partial[(std::size_t)k * L + c]);
    worst = fmaxf(worst, ppr_finish<L>(s, long_rows[r], c, seed, seed_term, acc));
  }
  ppr_flush<L>(worst, c, s_diff, s.ctr);
}

/// Stage one of D: a lane group per chunk of the dangling list, sequentially in list order.
template <int L>
__global__ void __launch_bounds__(PPR_BLOCK)
    ppr_dangling_kernel(const float* p, const int32_t* list, int32_t count, float* dpart) {
  int group, c;
  ppr_place<L>(group, c);
  constexpr int ROWS = ppr_shape_t<L>::groups;
  const int64_t chunks = ((int64_t)count + PPR_DANGLING_CHUNK - 1) / PPR_DANGLING_CHUNK;
  for (int64_t j0 = (int64_t)blockIdx.x * ROWS; j0 < chunks; j0 += (int64_t)gridDim.x * ROWS) {
    const int64_t j = j0 + group;
    if (j >= chunks)
      continue;
    const int32_t lo = (int32_t)(j * PPR_DANGLING_CHUNK);
    const int32_t hi = (int32_t)min((int64_t)count, (int64_t)lo + PPR_DANGLING_CHUNK);
    float acc = 0.0f;
    int32_t i = lo;
    for (; i + PPR_FLIGHT <= hi; i += PPR_FLIGHT) {
      float x[PPR_FLIGHT];
#pragma unroll
      for (int k = 0; k < PPR_FLIGHT; ++k)
        x[k] = p[(std::size_t)list[i + k] * L + c];
#pragma unroll
      for (int k = 0; k < PPR_FLIGHT; ++k)
        acc = __fadd_rn(acc, x[k]);
    }
    for (; i < hi; ++i)
      acc = __fadd_rn(acc, p[(std::size_t)list[i] * L + c]);
    dpart[(std::size_t)j * L + c] = acc;
  }
}

/// The hand-off of iteration t: one wavefront, lane = column, last in its batch of launches.  maxdiff
/// was changed by atomics: it is read and cleared past the caches.
__global__ void ppr_publish_kernel(ppr_counters_t* ctr, const float* dpart, int32_t chunks, int L, int width,
                                   int32_t t, float tol, unsigned long long* mirror, int sequence_slot,
                                   unsigned long long sequence) {
  const int c = threadIdx.x;
  const unsigned long long frozen = ctr->frozen;
  if (c < L) {  // stage two of D: the chunk sums in chunk order
    float d = 0.0f;
    for (int32_t j = 0; j < chunks; ++j)
      d = __fadd_rn(d, dpart[(std::size_t)j * L + c]);
    ctr->dangling[c] = d;
  }
  bool stops = false;
  if (c < PPR_BATCH) {
    const unsigned bits = __hip_atomic_exchange(&ctr->maxdiff[c], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c < width && !((frozen >> c) & 1)) {
      const float diff = __uint_as_float(bits);
      ctr->iterations[c] = t;
      ctr->residual[c] = diff;
      stops = tol > 0.0f && diff < tol;
    }
  }
  const unsigned long long now = frozen | __ballot(stops);
  if (c == 0) {
    ctr->frozen = now;
    mirror[PM_FROZEN] = now;
    stamp_handoff(mirror, sequence_slot, sequence);
  }
}

/// Delivery: p[V][L] to rows [0, width) of `out` ([width][V]), PPR_TILE vertices at a time through
/// LDS, both sides coalesced; counts the values > 0 per column.
template <int L>
__global__ void __launch_bounds__(PPR_BLOCK)
    ppr_deliver_kernel(const float* p, int32_t n, int width, float* out, ppr_counters_t* ctr) {
  __shared__ float s_tile[PPR_TILE][L + 1];
  constexpr int WAVES = PPR_BLOCK / wave_size;
  constexpr int TRIPS = (L + WAVES - 1) / WAVES;
  const int tid = threadIdx.x, wave = tid / wave_size, lane = tid % wave_size;
  unsigned count[TRIPS];
#pragma unroll
  for (int k = 0; k < TRIPS; ++k)
    count[k] = 0;
  const int64_t tiles = ((int64_t)n + PPR_TILE - 1) / PPR_TILE;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t v0 = tile * PPR_TILE;
    const int rows = (int)min((int64_t)PPR_TILE, (int64_t)n - v0);
    const float* src = p + (std::size_t)v0 * L;
    for (int i = tid; i < rows * L; i += PPR_BLOCK)
      s_tile[i / L][i % L] = src[i];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TRIPS; ++k) {
      const int c = wave + k * WAVES;  // the same in every lane of the wavefront
      if (c < width) {
        float x = 0.0f;
        if (lane < rows) {
          x = s_tile[lane][c];
          out[(std::size_t)c * (std::size_t)n + (std::size_t)(v0 + lane)] = x;
        }
        count[k] += (unsigned)__popcll(__ballot(x > 0.0f));
      }
    }
    __syncthreads();  // the next tile rewrites s_tile
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < TRIPS; ++k) {
      const int c = wave + k * WAVES;
      if (c < width && count[k])
        atomicAdd(&ctr->nonzero[c], (unsigned long long)count[k]);
    }
  }
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

/**
 * @file color_kernels.hxx
 * @brief Graph colouring (grx_color): greedy colouring in largest-degree-first order by
 * Jones-Plassmann, data-driven.
 *
 * Order: key(v) = (deg(v) << 32) | fmix32(v), recomputed from ap and the id wherever it is needed.
 * u precedes v when u != v, u is named by row v and key(u) > key(v).  State: pending[V] (entries of
 * row v that name a predecessor still uncoloured), color[V] (-1 until coloured) and one append-only
 * queue[V].  A vertex is queued exactly once, by whoever takes its pending to 0, so a generation is
 * a range [head, tail) of the queue: generation g holds the vertices of depth g in the priority DAG.
 *
 *   color_init_kernel      all rows, a chunk of COLOR_BLOCK consecutive vertices per workgroup
 *                          (flat_walk): pending[v] = entries naming a predecessor, color[v] = -1,
 *                          vertices with pending 0 are queued (generation 1).  Rows above `big_row`
 *                          are cut into segments (push_big_segments) ...
 *   color_init_big_kernel  ... counted a workgroup per segment ...
 *   color_ready_kernel     ... and queued when they have no predecessor.
 *   color_wide_kernel      one generation, a chunk of at most COLOR_BLOCK queued vertices per
 *                          workgroup, their rows flattened over its threads.  ONE walk classifies
 *                          every entry (v, u): u precedes v -> color[u] goes into v's mask; v
 *                          precedes u -> atomic_sub(pending[u], 1), and the one that returns 1
 *                          appends u behind tail.  Rows longer than `big_row` go to a list ...
 *   color_big_kernel       ... and get a workgroup each.
 *   color_narrow_kernel    ONE workgroup that runs consecutive small generations by itself, then
 *                          hands the counters to the host: it ends every batch of launches.
 *
 * Visibility of color[v].  Whoever takes pending[u] to 0 only QUEUES u: u reads the colours of its
 * predecessors in the next generation.  Between the wide / big kernels of one generation and the
 * kernels of the next lies a kernel boundary, so they use plain loads and stores.  Inside the narrow
 * kernel, which is one workgroup, the colour (and the queue slot) is stored past the L1 at agent
 * scope, the generations are separated by __syncthreads() (a workgroup-scope release: the wave
 * waits for its stores before the barrier) and the next generation loads past the L1.  No kernel
 * reads a colour written by another workgroup of the same launch.
 *
 * Smallest absent colour.  Colours below 64 go into a 64-bit mask per queued vertex (in LDS: the
 * entries of its row are spread over the workgroup's lanes; its owner thread takes the mask into a
 * register when the walk is over).  With at most 64 predecessors the mask decides.  A vertex whose
 * mask is full is walked again by the whole workgroup with an LDS bitmap over the window
 * [64, 64 + W), then [64 + W, 64 + 2W) ... until a window has a gap: mex <= predecessors, so at
 * most deg / W + 1 windows.  A big row is walked that way from window [0, W) on.
 */
#pragma once

#include <gunrock/hip/kernels/generation_queue.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int COLOR_BLOCK = 256;
constexpr int COLOR_NARROW_BLOCK = 1024;   // also the narrow kernel's capacity in vertices
constexpr int COLOR_NARROW_EDGES = 16384;  // default: generations with more entries go wide
constexpr int COLOR_BIG_ROW = 4096;        // default: longer rows get a workgroup of their own
constexpr int COLOR_BIG_SEGMENT = 4096;    // the init pass cuts them into segments of this many
constexpr int COLOR_MEX_WINDOW = 2048;     // colours per LDS window: default and largest
constexpr int COLOR_NO_COLOR = 0x7fffffff;

/// Device counters of one grx_color call (big_n: segments during init, rows in a generation).
struct color_counters_t : queue_counters_t {
  int max_color, pad;              // largest colour written
  unsigned long long generations;  // generations the narrow kernel ran
};
/// The mirror words the host reads per hand-off besides the queue's.
enum { CL_MAX_COLOR = GQ_WORDS, CL_GENERATIONS, CL_WORDS };

__device__ __forceinline__ unsigned long long color_key(const int32_t* ap, int32_t v) {
  return ((unsigned long long)(unsigned)(ap[v + 1] - ap[v]) << 32) | fmix32((unsigned)v);
}

/// One entry naming a vertex w that the row's vertex precedes (`down` lanes hold one): one
/// predecessor less; every lane of the wavefront calls it.
template <bool NARROW>
__device__ __forceinline__ void color_notify(bool down, int32_t w, const int32_t* ap, int32_t* pending,
                                             const queue_sink_t& sink, unsigned long long& dsum) {
  bool ready = false;
  if (down)
    ready = atomicSub(&pending[w], 1) == 1;
  queue_append<NARROW>(ready, w, ap, sink, dsum);
}

template <bool NARROW>
__device__ __forceinline__ int32_t color_of(const int32_t* color, int32_t u) {
  return NARROW ? load_relaxed(color + u) : color[u];
}
template <bool NARROW>
__device__ __forceinline__ void color_set(int32_t* color, int32_t v, int32_t c) {
  if (NARROW)
    store_relaxed(color + v, c);
  else
    color[v] = c;
}

/// The smallest colour >= base absent among v's predecessors, by the whole workgroup: an LDS bitmap
/// over [base, base + window), moved up until a window has a gap.  With `relax` the first walk also
/// tells the vertices v precedes.  Valid in every thread; `window`: a multiple of 32, at most
/// COLOR_MEX_WINDOW; `s_bits`: COLOR_MEX_WINDOW / 32 words.  Ends with a barrier.
template <int BLOCK, bool NARROW>
__device__ __forceinline__ int32_t color_block_mex(const int32_t* ap, const int32_t* aj, const int32_t* color,
                                                   int32_t* pending, int32_t v, int32_t base, int32_t window,
                                                   bool relax, const queue_sink_t& sink, unsigned* s_bits,
                                                   int32_t* s_found, unsigned long long& dsum) {
  const int tid = threadIdx.x;
  const int32_t lo = ap[v], hi = ap[v + 1];
  const unsigned long long kv = color_key(ap, v);
  const int words = window / 32;
  // every window without a gap holds `window` distinct predecessor colours: at most deg / window trips
  for (;; base += window) {
    for (int i = tid; i < words; i += BLOCK)
      s_bits[i] = 0;
    if (tid == 0)
      *s_found = COLOR_NO_COLOR;
    __syncthreads();
    // whole wavefronts run every trip: the ballot of color_notify sees all 64 lanes
    for (int64_t e0 = lo; e0 < hi; e0 += BLOCK) {
      const int64_t e = e0 + tid;
      bool down = false;
      int32_t u = 0;
      if (e < hi) {
        u = aj[e];
        if (u != v) {
          if (color_key(ap, u) > kv) {
            const int32_t c = color_of<NARROW>(color, u) - base;
            if ((unsigned)c < (unsigned)window)
              atomicOr(&s_bits[c >> 5], 1u << (c & 31));
          } else {
            down = relax;
          }
        }
      }
      if (relax)  // uniform
        color_notify<NARROW>(down, u, ap, pending, sink, dsum);
    }
    relax = false;
    __syncthreads();
    for (int i = tid; i < words; i += BLOCK) {
      const unsigned absent = ~s_bits[i];
      if (absent)
        atomicMin(s_found, base + i * 32 + (__ffs((int)absent) - 1));
    }
    __syncthreads();
    const int32_t found = *s_found;
    __syncthreads();  // the next window, or the caller, rewrites s_found and the bitmap
    if (found != COLOR_NO_COLOR)
      return found;
  }
}

/// LDS of a workgroup that colours chunks of BLOCK queued vertices.
template <int BLOCK>
struct color_chunk_lds_t {
  unsigned long long key[BLOCK];   // the owners' keys
  unsigned long long mask[BLOCK];  // colours 0..63 of the owners' predecessors
  int32_t pre[BLOCK], base[BLOCK], vert[BLOCK], over[BLOCK];
  int32_t wave[BLOCK / wave_size + 1];
  unsigned bits[COLOR_MEX_WINDOW / 32];
  int32_t found;
  int n_over;
};

/// Colour queue[a, b) (b - a <= BLOCK) with the whole workgroup and tell the vertices they precede.
/// Returns the entries classified.  Ends with a barrier.
template <int BLOCK, bool NARROW>
__device__ __forceinline__ int32_t color_chunk(const int32_t* ap, const int32_t* aj, int32_t* pending, int32_t* color,
                                               int32_t a, int32_t b, int32_t big_row, int32_t* big, int32_t window,
                                               color_counters_t* ctr, const queue_sink_t& sink,
                                               color_chunk_lds_t<BLOCK>& s, int32_t& mx, unsigned long long& dsum) {
  const int tid = threadIdx.x;
  int32_t v = -1;
  s.mask[tid] = 0;
  if (tid == 0)
    s.n_over = 0;
  const int32_t P = queue_walk<BLOCK, NARROW>(
      ap, sink.queue, a, b, s.pre, s.base, s.wave,
      [&](int32_t u, int32_t, int32_t& d) {
        s.key[tid] = ((unsigned long long)(unsigned)d << 32) | fmix32((unsigned)u);
        if (NARROW || !queue_divert_big(u, d, big_row, big, &ctr->big_n))
          v = u;
        s.vert[tid] = v;
      },
      [&](bool live, int o, int32_t e) {
        bool down = false;
        int32_t u = 0;
        if (live) {
          u = aj[e];
          if (u != s.vert[o]) {
            if (color_key(ap, u) > s.key[o]) {
              const int32_t c = color_of<NARROW>(color, u);
              // neighbouring lanes share an owner and often a colour: test before the atomic
              if ((unsigned)c < 64u && !((__hip_atomic_load(&s.mask[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> c) & 1))
                atomicOr(&s.mask[o], 1ull << c);
            } else {
              down = true;
            }
          }
        }
        color_notify<NARROW>(down, u, ap, pending, sink, dsum);
      });
  if (v >= 0) {
    const unsigned long long absent = ~s.mask[tid];
    if (absent) {
      const int32_t c = __ffsll((long long)absent) - 1;
      color_set<NARROW>(color, v, c);
      mx = max(mx, c);
    } else {
      s.over[atomicAdd(&s.n_over, 1)] = v;
    }
  }
  __syncthreads();
  const int n_over = s.n_over;
  for (int i = 0; i < n_over; ++i) {  // colours 0..63 all taken: the windows above them
    const int32_t w = s.over[i];
    const int32_t c = color_block_mex<BLOCK, NARROW>(ap, aj, color, pending, w, 64, window, false, sink, s.bits,
                                                     &s.found, dsum);
    if (tid == 0) {
      color_set<NARROW>(color, w, c);
      mx = max(mx, c);
    }
  }
  __syncthreads();  // the next chunk rewrites the LDS
  return P;
}

/// Flush a thread's largest colour: one atomic per wavefront.
__device__ __forceinline__ void color_flush_max(int32_t mx, int* max_color) {
  mx = wave_max(mx);
  if (lane_id() == 0 && mx > 0)
    atomicMax(max_color, mx);
}

__global__ void __launch_bounds__(COLOR_BLOCK)
    color_init_kernel(const int32_t* ap, const int32_t* aj, int32_t n, int32_t big_row, int32_t* pending,
                      int32_t* color, int32_t* queue, int2* big, color_counters_t* ctr) {
  __shared__ int32_t s_pre[COLOR_BLOCK], s_base[COLOR_BLOCK], s_wave[COLOR_BLOCK / wave_size + 1];
  __shared__ int32_t s_count[COLOR_BLOCK];
  __shared__ unsigned long long s_key[COLOR_BLOCK];
  const int tid = threadIdx.x;
  const queue_sink_t sink{queue, n, &ctr->tail, &ctr->degsum};
  unsigned long long dsum = 0, walked = 0, rows = 0;
  unsigned mxrow = 0;
  for (int64_t v0 = (int64_t)blockIdx.x * COLOR_BLOCK; v0 < n; v0 += (int64_t)gridDim.x * COLOR_BLOCK) {
    const int64_t v = v0 + tid;
    int32_t lo = 0, d = 0;
    bool is_big = false;
    unsigned long long kv = 0;
    if (v < n) {
      lo = ap[v];
      d = max(ap[v + 1] - lo, 0);
      kv = ((unsigned long long)(unsigned)d << 32) | fmix32((unsigned)v);
      rows += d > 0;
      mxrow = max(mxrow, (unsigned)d);
      if (d > big_row) {
        push_big_segments<COLOR_BIG_SEGMENT>(&ctr->big_n, big, (int32_t)v, d);
        walked += (unsigned long long)d;
        is_big = true;
        d = 0;
      }
    }
    s_count[tid] = 0;
    s_key[tid] = kv;
    const int32_t P = flat_walk<COLOR_BLOCK>(d, lo, s_pre, s_base, s_wave, [&](int o, int32_t e) {
      const int32_t u = aj[e];
      if (u != (int32_t)v0 + o && color_key(ap, u) > s_key[o])
        atomicAdd(&s_count[o], 1);
    });
    walked += (unsigned long long)(tid == 0 ? P : 0);
    // s_count is complete behind flat_walk's trailing barrier (P == 0: nobody wrote it)
    bool ready = false;
    if (v < n) {
      const int32_t count = s_count[tid];
      pending[v] = count;  // a big row: 0, its segments add to it in the next kernel
      color[v] = -1;
      ready = !is_big && count == 0;
    }
    queue_append<false>(ready, (int32_t)v, ap, sink, dsum);
  }
  queue_flush(dsum, &ctr->degsum);
  rows = wave_sum(rows);
  walked = wave_sum(walked);
  mxrow = wave_max(mxrow);
  if (lane_id() == 0) {
    if (rows)
      atomicAdd(&ctr->nonempty, rows);
    if (walked)
      atomicAdd(&ctr->edges, walked);
    if (mxrow)
      atomicMax(&ctr->max_row, mxrow);
  }
}

/// The segments of the long rows, one workgroup each: pending[v] += entries naming a predecessor.
__global__ void __launch_bounds__(COLOR_BLOCK)
    color_init_big_kernel(const int32_t* ap, const int32_t* aj, int32_t* pending, const int2* big,
                          const color_counters_t* ctr) {
  __shared__ int32_t s_sum[COLOR_BLOCK / wave_size];
  const int32_t items = ctr->big_n;  // written by the init kernel before this one; constant here
  for (int32_t i = blockIdx.x; i < items; i += gridDim.x) {
    const int2 item = big[i];  // {vertex, segment of its row}
    const int32_t v = item.x;
    const unsigned long long kv = color_key(ap, v);
    const int64_t lo = (int64_t)ap[v] + (int64_t)item.y * COLOR_BIG_SEGMENT;
    const int64_t hi = min((int64_t)ap[v + 1], lo + COLOR_BIG_SEGMENT);
    int32_t count = 0;
    for (int64_t e = lo + threadIdx.x; e < hi; e += COLOR_BLOCK) {
      const int32_t u = aj[e];
      count += u != v && color_key(ap, u) > kv;
    }
    count = block_sum<COLOR_BLOCK>(count, s_sum);
    if (threadIdx.x == 0 && count)
      atomicAdd(&pending[v], count);
    __syncthreads();  // the next item rewrites s_sum
  }
}

/// One workgroup: the long rows without a predecessor join generation 1.
__global__ void __launch_bounds__(COLOR_NARROW_BLOCK)
    color_ready_kernel(const int32_t* ap, const int32_t* pending, int32_t* queue, int32_t n, const int2* big,
                       color_counters_t* ctr) {
  const queue_sink_t sink{queue, n, &ctr->tail, &ctr->degsum};
  const int32_t items = ctr->big_n;
  unsigned long long dsum = 0;
  // whole wavefronts run every trip: the ballot of queue_append sees all 64 lanes
  for (int32_t i0 = 0; i0 < items; i0 += COLOR_NARROW_BLOCK) {
    const int32_t i = i0 + threadIdx.x;
    bool ready = false;
    int32_t v = 0;
    if (i < items) {
      const int2 item = big[i];
      v = item.x;
      ready = item.y == 0 && pending[v] == 0;
    }
    queue_append<false>(ready, v, ap, sink, dsum);
  }
  queue_flush(dsum, &ctr->degsum);
  __syncthreads();
  if (threadIdx.x == 0)
    ctr->big_n = 0;  // the generations' list starts empty
}

__global__ void __launch_bounds__(COLOR_BLOCK)
    color_wide_kernel(const int32_t* ap, const int32_t* aj, int32_t* pending, int32_t* color, int32_t* queue, int32_t n,
                      int32_t head, int32_t tail, int32_t chunk, int32_t big_row, int32_t* big, int32_t window,
                      color_counters_t* ctr) {
  __shared__ color_chunk_lds_t<COLOR_BLOCK> s;
  const queue_sink_t sink{queue, n, &ctr->tail, &ctr->degsum};
  int32_t mx = 0;
  unsigned long long dsum = 0, walked = 0;
  for (int64_t a = head + (int64_t)blockIdx.x * chunk; a < tail; a += (int64_t)gridDim.x * chunk) {
    const int32_t b = (int32_t)min((int64_t)tail, a + chunk);
    walked += (unsigned long long)color_chunk<COLOR_BLOCK, false>(ap, aj, pending, color, (int32_t)a, b, big_row, big,
                                                                 window, ctr, sink, s, mx, dsum);
  }
  color_flush_max(mx, &ctr->max_color);
  queue_flush(dsum, &ctr->degsum);
  if (threadIdx.x == 0 && walked)
    atomicAdd(&ctr->edges, walked);
}

/// The rows on the big list, a workgroup each: one walk tells the vertices the row's vertex
/// precedes and fills the first window; further windows only when that one is full.
__global__ void __launch_bounds__(COLOR_BLOCK)
    color_big_kernel(const int32_t* ap, const int32_t* aj, int32_t* pending, int32_t* color, int32_t* queue, int32_t n,
                     const int32_t* big, int32_t window, color_counters_t* ctr) {
  __shared__ unsigned s_bits[COLOR_MEX_WINDOW / 32];
  __shared__ int32_t s_found;
  const queue_sink_t sink{queue, n, &ctr->tail, &ctr->degsum};
  const int32_t rows = ctr->big_n;  // written by the wide kernel before this one; constant here
  int32_t mx = 0;
  unsigned long long dsum = 0, walked = 0;
  for (int32_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const int32_t v = big[r];
    const int32_t c =
        color_block_mex<COLOR_BLOCK, false>(ap, aj, color, pending, v, 0, window, true, sink, s_bits, &s_found, dsum);
    if (threadIdx.x == 0) {
      color[v] = c;
      mx = max(mx, c);
      walked += (unsigned long long)(ap[v + 1] - ap[v]);
    }
  }
  color_flush_max(mx, &ctr->max_color);
  queue_flush(dsum, &ctr->degsum);
  if (threadIdx.x == 0 && walked)
    atomicAdd(&ctr->edges, walked);
}

/// One workgroup: generations while they are small, then the hand-off to the host.
__global__ void __launch_bounds__(COLOR_NARROW_BLOCK)
    color_narrow_kernel(const int32_t* ap, const int32_t* aj, int32_t* pending, int32_t* color, int32_t* queue,
                        int32_t n, int32_t max_vertices, unsigned long long max_edges, int32_t window,
                        color_counters_t* ctr, unsigned long long* mirror, int sequence_slot,
                        unsigned long long sequence) {
  __shared__ color_chunk_lds_t<COLOR_NARROW_BLOCK> s;
  __shared__ int s_tail, s_max;
  __shared__ unsigned long long s_dsum;
  if (threadIdx.x == 0)
    s_max = ctr->max_color;
  int32_t mx = 0;
  const narrow_result_t r = narrow_generations(
      ctr, queue, n, max_vertices, max_edges, &s_tail, &s_dsum,
      [&](int32_t head, int32_t tail, const queue_sink_t& sink, unsigned long long& dsum) {
        return color_chunk<COLOR_NARROW_BLOCK, true>(ap, aj, pending, color, head, tail, 0, nullptr, window, ctr, sink,
                                                     s, mx, dsum);
      });
  color_flush_max(mx, &s_max);
  __syncthreads();
  if (threadIdx.x == 0) {
    // no other kernel of the call runs beside this one
    ctr->edges += r.walked;
    ctr->generations += r.generations;
    ctr->max_color = s_max;
    mirror[CL_MAX_COLOR] = (unsigned long long)s_max;
    mirror[CL_GENERATIONS] = ctr->generations;
    queue_publish(ctr, mirror, sequence_slot, sequence, r.head, r.tail, r.degsum);
  }
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

/**
 * @file bfs_multi_kernels.hxx
 * @brief Multi-source BFS (grx_bfs_multi): up to 64 searches share one walk of the edge stream and
 * one hand-off per level ("The More the Merrier", Then et al., VLDB 2014).  Bit i of every 64-bit
 * word stands for source i of the batch.
 *
 * State per vertex: seen[V] (the searches that have a depth for it) and two frontier arrays that
 * take turns, front[V] (the searches that reached it AT the current level L) and next[V] (level
 * L + 1 while it is gathered).  Per level an ACTIVE LIST holds each vertex with a non-zero front word
 * exactly once; there are two lists of V slots, which take turns too.  Invariants between levels:
 *
 *   front[v] != 0  iff  v is on the active list, and front[v] & ~seen[v] == 0;
 *   next[v] == 0 for every v (the level before the last one left it so: bfsm_update_kernel clears
 *   the words of the list it was built from), and the next list is empty.
 *
 * A level is expanded in one of two forms, both of which end with the invariants restored for L + 1:
 *
 *   PUSH  bfsm_push_kernel     the active list's rows flattened over the workgroup (queue_walk: whole
 *                              wavefronts, consecutive threads on consecutive entries).  Entry (u, v):
 *                              m = front[u] & ~seen[v] & ~next[v], two plain pre-tests (seen does not
 *                              change in the kernel and next only grows: a stale read errs towards
 *                              the atomic); when m != 0 one atomicOr(&next[v], m), and the lane that
 *                              gets 0 back appends v: once per level, so V slots hold.  Rows above
 *                              `big_row` are cut into segments (push_big_segments) ...
 *         bfsm_push_big_kernel ... a workgroup per segment.
 *         bfsm_update_kernel   the next list: n = next[v] & ~seen[v] (every OR left the seen bits
 *                              out, so n is the word as it stands), seen[v] |= n, then bfsm_settle.
 *   PULL  bfsm_pull_kernel     every vertex with ~seen[v] & mask != 0 ORs the front words of its
 *                              in-neighbours into an LDS word (flattened over the workgroup as well)
 *                              until the word covers what it lacks; n = acc & ~seen[v]; next[v] = n,
 *                              seen[v] |= n, append, bfsm_settle.  No atomics on next.  It reads
 *                              front while it writes next: hence two arrays.  In-rows above `big_row`
 *                              are listed ...
 *         bfsm_pull_big_kernel ... and take a workgroup each, with an OR-reduction.
 *         bfsm_update_kernel   with nothing to settle: it clears the old list's words only.
 *
 * bfsm_settle is what a newly reached (vertex, bits) pair costs whichever form found it: for every
 * bit of the wavefront's union, the lanes that have it store depth[bit * V + v] = level (a fixed bit
 * at a time across the lanes, so a run of neighbouring vertices is a run of neighbouring addresses)
 * and one lane adds the ballot's popcount to an LDS counter; a workgroup ends with one global atomic
 * per non-zero counter, spread over BFSM_REPLICAS copies of the counters.  bfsm_publish_kernel folds
 * them into the totals (reached, level * count, last non-empty level: integers, so order cannot
 * matter), hands the next list's length, degree sum and longest row to the host and stamps.
 *
 * No kernel waits on another workgroup.  Every list store is guarded by `at < n`; the big lists are
 * sized by the host from nnz (a vertex is on a level's list once).  Hook: GRX_BFSM_BIG_ROW.
 */
#pragma once

#include <gunrock/hip/kernels/generation_queue.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int BFSM_BLOCK = 256;
constexpr int BFSM_BATCH = 64;           // searches per batch: the bits of a word
constexpr int BFSM_BIG_ROW = 4096;       // default: longer rows go to whole workgroups
constexpr int BFSM_BIG_SEGMENT = 4096;   // a pushed long row is cut into segments of this many
constexpr int BFSM_REPLICAS = 16;        // copies of the per-level counters (a line retires atomics one by one)

using bfsm_word_t = unsigned long long;

/// Device counters of one batch.
struct bfsm_counters_t {
  int tail;                   // vertices on the next list
  int big_n;                  // items on the big list of the kernel that runs
  unsigned max_row;           // longest row of the next list
  int pad;
  unsigned long long degsum;  // entries of the next list's rows
  unsigned long long read;    // in-row entries the pull kernels read, all levels
  int level_count[BFSM_REPLICAS][BFSM_BATCH];  // per bit: vertices reached at the level being gathered
  unsigned long long reached[BFSM_BATCH], depth_sum[BFSM_BATCH];
  int eccentricity[BFSM_BATCH];
};
/// The mirror words the host reads per hand-off.
enum { BM_TAIL = 0, BM_DEGSUM, BM_MAX_ROW, BM_READ, BM_WORDS };

/// The sources of a batch, by value.
struct bfsm_sources_t {
  int32_t v[BFSM_BATCH];
};

/// One direction of the graph.
struct bfsm_rows_t {
  const int32_t* ap;
  const int32_t* aj;
};

/// Where newly reached vertices go.
struct bfsm_out_t {
  bfsm_word_t* seen;
  bfsm_word_t* next;   // level + 1's frontier words
  int32_t* depth;      // the batch's rows, [bits][n]; NULL: summaries only
  int32_t* list;       // the next list, n slots
  const int32_t* ap;   // out-rows: the degree sum of the next list
  int32_t n;
  int32_t level;       // the depth being handed out
  bfsm_counters_t* ctr;
};

__device__ __forceinline__ bfsm_word_t bfsm_wave_or(bfsm_word_t x) {
#pragma unroll
  for (int d = wave_size / 2; d > 0; d >>= 1)
    x |= __shfl_xor(x, d, wave_size);
  // the same in every lane: say so, the loop over its bits is then scalar.  The builtin returns a
  // signed int: through unsigned, or bit 31 of the low half would fill the high half
  const unsigned high = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x >> 32));
  const unsigned low = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x);
  return ((bfsm_word_t)high << 32) | (bfsm_word_t)low;
}

/// Append v for the lanes with `ready` (queue_append's pattern: one atomic per wavefront); every lane
/// of the wavefront calls it.
__device__ __forceinline__ void bfsm_append(bool ready, int32_t v, int32_t* list, int32_t n, int* tail) {
  const unsigned long long m = __ballot(ready);
  if (m) {
    const int first = __ffsll((long long)m) - 1;
    int32_t base = 0;
    if (lane_id() == first)
      base = atomicAdd(tail, __popcll(m));
    base = __shfl(base, first, wave_size);
    if (ready) {
      const int32_t at = base + rank_in_mask(m);
      if (at < n)  // a vertex is listed once per level, so this holds; it guards the store all the same
        list[at] = v;
    }
  }
}

/// Entry (u, v) of a pushed row, f = front[u].  True for the one lane that is to append v.
__device__ __forceinline__ bool bfsm_relax(bfsm_word_t f, int32_t v, const bfsm_word_t* seen, bfsm_word_t* next) {
  bfsm_word_t m = f & ~seen[v];
  if (!m)
    return false;
  m &= ~next[v];
  if (!m)
    return false;
  return atomicOr(&next[v], m) == 0;
}

/// Lanes with `has` reached v for the searches in n (!= 0) at o.level: depths, counts, the degree
/// sum and longest row of the next list.  Every lane of the wavefront calls it.  `s_count`: the
/// workgroup's BFSM_BATCH counters in LDS.
__device__ __forceinline__ void bfsm_settle(bool has, int32_t v, bfsm_word_t n, const bfsm_out_t& o, int* s_count,
                                            unsigned long long& dsum, unsigned& mxrow) {
  if (!has)
    n = 0;
  bfsm_word_t any = bfsm_wave_or(n);
  if (!any)
    return;
  if (n) {
    const unsigned d = (unsigned)(o.ap[v + 1] - o.ap[v]);
    dsum += d;
    mxrow = max(mxrow, d);
  }
  const bool first = lane_id() == 0;
  while (any) {
    const int i = __ffsll((long long)any) - 1;
    any &= any - 1;
    const bool on = (n >> i) & 1;
    const unsigned long long who = __ballot(on);
    if (on && o.depth)
      o.depth[(std::size_t)i * (std::size_t)o.n + (std::size_t)v] = o.level;
    if (first)
      atomicAdd(&s_count[i], __popcll(who));
  }
}

/// What ends a settling kernel: one global atomic per non-zero counter, and the list's facts.
/// Every thread of the workgroup calls it.
__device__ __forceinline__ void bfsm_flush(int* s_count, unsigned long long dsum, unsigned mxrow,
                                           bfsm_counters_t* ctr) {
  __syncthreads();
  if (threadIdx.x < BFSM_BATCH) {
    const int c = s_count[threadIdx.x];
    if (c)
      atomicAdd(&ctr->level_count[blockIdx.x % BFSM_REPLICAS][threadIdx.x], c);
  }
  dsum = wave_sum(dsum);
  mxrow = wave_max(mxrow);
  if (lane_id() == 0) {
    if (dsum)
      atomicAdd(&ctr->degsum, dsum);
    if (mxrow)
      atomicMax(&ctr->max_row, mxrow);
  }
}

/// Level 0 of a batch: bit i into the word of source i.  One wavefront.
__global__ void bfsm_seed_kernel(bfsm_sources_t src, int bits, bfsm_word_t* next, int32_t* list, int32_t n,
                                 bfsm_counters_t* ctr) {
  const int lane = threadIdx.x;
  bool claim = false;
  int32_t s = 0;
  if (lane < bits) {
    s = src.v[lane];
    claim = atomicOr(&next[s], (bfsm_word_t)1 << lane) == 0;  // a vertex named twice is listed once
  }
  bfsm_append(claim, s, list, n, &ctr->tail);
}

/// PUSH: active[0, count) in chunks of at most `chunk` <= BFSM_BLOCK vertices per workgroup.
__global__ void __launch_bounds__(BFSM_BLOCK)
    bfsm_push_kernel(bfsm_rows_t out, const int32_t* active, int32_t count, int32_t chunk, const bfsm_word_t* front,
                     const bfsm_word_t* seen, bfsm_word_t* next, int32_t* list, int32_t n, int32_t big_row, int2* big,
                     bfsm_counters_t* ctr) {
  __shared__ int32_t s_pre[BFSM_BLOCK], s_base[BFSM_BLOCK], s_wave[BFSM_BLOCK / wave_size + 1];
  __shared__ bfsm_word_t s_front[BFSM_BLOCK];
  const int tid = threadIdx.x;
  for (int64_t a = (int64_t)blockIdx.x * chunk; a < count; a += (int64_t)gridDim.x * chunk) {
    const int32_t b = (int32_t)min((int64_t)count, a + chunk);
    queue_walk<BFSM_BLOCK, false>(
        out.ap, active, (int32_t)a, b, s_pre, s_base, s_wave,
        [&](int32_t u, int32_t, int32_t& d) {
          s_front[tid] = front[u];
          if (d > big_row) {
            push_big_segments<BFSM_BIG_SEGMENT>(&ctr->big_n, big, u, d);
            d = 0;
          }
        },
        [&](bool live, int o, int32_t e) {
          const int32_t v = live ? out.aj[e] : 0;
          const bool claim = live && bfsm_relax(s_front[o], v, seen, next);
          bfsm_append(claim, v, list, n, &ctr->tail);
        });
  }
}

/// PUSH: the segments of the long rows, a workgroup each.
__global__ void __launch_bounds__(BFSM_BLOCK)
    bfsm_push_big_kernel(bfsm_rows_t out, const bfsm_word_t* front, const bfsm_word_t* seen, bfsm_word_t* next,
                         int32_t* list, int32_t n, const int2* big, bfsm_counters_t* ctr) {
  const int32_t items = ctr->big_n;  // written by the push kernel before this one; constant here
  for (int32_t i = blockIdx.x; i < items; i += gridDim.x) {
    const int2 item = big[i];  // {vertex, segment of its row}
    const bfsm_word_t f = front[item.x];
    const int64_t lo = (int64_t)out.ap[item.x] + (int64_t)item.y * BFSM_BIG_SEGMENT;
    const int64_t hi = min((int64_t)out.ap[item.x + 1], lo + BFSM_BIG_SEGMENT);
    // whole wavefronts run every trip: the ballot of bfsm_append sees all 64 lanes
    for (int64_t e0 = lo; e0 < hi; e0 += BFSM_BLOCK) {
      const int64_t e = e0 + threadIdx.x;
      const int32_t v = e < hi ? out.aj[e] : 0;
      const bool claim = e < hi && bfsm_relax(f, v, seen, next);
      bfsm_append(claim, v, list, n, &ctr->tail);
    }
  }
}

/// Settle the next list (its length is the device's to know: the push kernels just wrote it) when
/// `settle`, and clear the front words of the list the level was expanded from.
__global__ void __launch_bounds__(BFSM_BLOCK)
    bfsm_update_kernel(bfsm_out_t o, int settle, bfsm_word_t* front, const int32_t* active, int32_t active_count) {
  __shared__ int s_count[BFSM_BATCH];
  const int tid = threadIdx.x;
  if (tid < BFSM_BATCH)
    s_count[tid] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * BFSM_BLOCK;
  unsigned long long dsum = 0;
  unsigned mxrow = 0;
  if (settle) {
    const int32_t count = min(o.ctr->tail, o.n);
    // whole wavefronts run every trip: bfsm_settle holds ballots
    for (int64_t t0 = (int64_t)blockIdx.x * BFSM_BLOCK; t0 < count; t0 += stride) {
      const int64_t t = t0 + tid;
      int32_t v = 0;
      bfsm_word_t nw = 0;
      if (t < count) {
        v = o.list[t];
        const bfsm_word_t sv = o.seen[v];
        nw = o.next[v] & ~sv;
        o.seen[v] = sv | nw;
      }
      bfsm_settle(nw != 0, v, nw, o, s_count, dsum, mxrow);
    }
  }
  for (int64_t t = (int64_t)blockIdx.x * BFSM_BLOCK + tid; t < active_count; t += stride)
    front[active[t]] = 0;
  bfsm_flush(s_count, dsum, mxrow, o.ctr);
}

/// PULL: every vertex that lacks a search of `mask`, BFSM_BLOCK consecutive vertices per workgroup.
__global__ void __launch_bounds__(BFSM_BLOCK)
    bfsm_pull_kernel(bfsm_rows_t in, const bfsm_word_t* front, bfsm_out_t o, bfsm_word_t mask, int32_t big_row,
                     int32_t* big) {
  __shared__ int32_t s_pre[BFSM_BLOCK], s_base[BFSM_BLOCK], s_wave[BFSM_BLOCK / wave_size + 1];
  __shared__ bfsm_word_t s_acc[BFSM_BLOCK], s_need[BFSM_BLOCK];
  __shared__ int s_count[BFSM_BATCH];
  const int tid = threadIdx.x;
  if (tid < BFSM_BATCH)
    s_count[tid] = 0;
  __syncthreads();
  unsigned long long dsum = 0, read = 0;
  unsigned mxrow = 0;
  for (int64_t v0 = (int64_t)blockIdx.x * BFSM_BLOCK; v0 < o.n; v0 += (int64_t)gridDim.x * BFSM_BLOCK) {
    const int64_t v = v0 + tid;
    bfsm_word_t sv = 0, need = 0;
    int32_t lo = 0, d = 0;
    if (v < o.n) {
      sv = o.seen[v];
      need = ~sv & mask;
      if (need) {
        lo = in.ap[v];
        d = in.ap[v + 1] - lo;
        if (d > big_row) {  // a workgroup of the next kernel gathers and settles it
          big[atomicAdd(&o.ctr->big_n, 1)] = (int32_t)v;
          d = 0;
          need = 0;
        }
      }
    }
    s_acc[tid] = 0;
    s_need[tid] = need;
    flat_walk<BFSM_BLOCK>(d, lo, s_pre, s_base, s_wave, [&](int ow, int32_t e) {
      const bfsm_word_t lacks = s_need[ow] & ~__hip_atomic_load(&s_acc[ow], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (!lacks)  // the row has given all it can: the rest of it stays unread
        return;
      ++read;
      const bfsm_word_t f = front[in.aj[e]] & lacks;
      if (f)
        atomicOr(&s_acc[ow], f);
    });
    // s_acc is complete behind flat_walk's trailing barrier (no entries: nobody else touched it)
    const bfsm_word_t nw = s_acc[tid] & need;
    if (nw) {
      o.seen[v] = sv | nw;
      o.next[v] = nw;
    }
    bfsm_append(nw != 0, (int32_t)v, o.list, o.n, &o.ctr->tail);
    bfsm_settle(nw != 0, (int32_t)v, nw, o, s_count, dsum, mxrow);
  }
  bfsm_flush(s_count, dsum, mxrow, o.ctr);
  read = wave_sum(read);
  if (lane_id() == 0 && read)
    atomicAdd(&o.ctr->read, read);
}

/// PULL: the listed long in-rows, a workgroup each; a wavefront stops once its lanes cover the lack.
__global__ void __launch_bounds__(BFSM_BLOCK)
    bfsm_pull_big_kernel(bfsm_rows_t in, const bfsm_word_t* front, bfsm_out_t o, bfsm_word_t mask, const int32_t* big) {
  __shared__ bfsm_word_t s_part[BFSM_BLOCK / wave_size];
  __shared__ int s_count[BFSM_BATCH];
  const int tid = threadIdx.x;
  if (tid < BFSM_BATCH)
    s_count[tid] = 0;
  __syncthreads();
  const int32_t rows = o.ctr->big_n;  // written by the pull kernel before this one; constant here
  unsigned long long dsum = 0, read = 0;
  unsigned mxrow = 0;
  for (int32_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const int32_t v = big[r];
    const bfsm_word_t sv = o.seen[v];
    const bfsm_word_t need = ~sv & mask;
    const int64_t lo = in.ap[v], hi = in.ap[v + 1];
    bfsm_word_t acc = 0;
    for (int64_t e0 = lo; e0 < hi; e0 += BFSM_BLOCK) {
      const int64_t e = e0 + tid;
      bfsm_word_t f = 0;
      if (e < hi) {
        f = front[in.aj[e]] & need;
        ++read;
      }
      acc |= bfsm_wave_or(f);
      if (!(need & ~acc))  // the same in every lane of the wavefront
        break;
    }
    if (lane_id() == 0)
      s_part[tid / wave_size] = acc;
    __syncthreads();
    if (tid < wave_size) {  // the first wavefront settles the row: lane 0 holds it
      bfsm_word_t nw = 0;
      if (tid == 0) {
        for (int w = 0; w < BFSM_BLOCK / wave_size; ++w)
          nw |= s_part[w];
        nw &= need;
        if (nw) {
          o.seen[v] = sv | nw;
          o.next[v] = nw;
        }
      }
      bfsm_append(nw != 0, v, o.list, o.n, &o.ctr->tail);
      bfsm_settle(nw != 0, v, nw, o, s_count, dsum, mxrow);
    }
    __syncthreads();  // the next row rewrites s_part
  }
  bfsm_flush(s_count, dsum, mxrow, o.ctr);
  read = wave_sum(read);
  if (lane_id() == 0 && read)
    atomicAdd(&o.ctr->read, read);
}

/// The hand-off of a level: one wavefront, last in its batch of launches.  Lane i folds the counts
/// of bit i at `level` into the totals; lane 0 hands the next list's facts over and empties the
/// lists for the level after it.  The counters were changed by atomics: they are read and cleared
/// past the caches.
__global__ void bfsm_publish_kernel(bfsm_counters_t* ctr, int32_t level, unsigned long long* mirror,
                                    int sequence_slot, unsigned long long sequence) {
  const int i = threadIdx.x;
  if (i < BFSM_BATCH) {
    unsigned long long c = 0;
    for (int r = 0; r < BFSM_REPLICAS; ++r)
      c += (unsigned long long)__hip_atomic_exchange(&ctr->level_count[r][i], 0, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
    if (c) {
      ctr->reached[i] += c;
      ctr->depth_sum[i] += c * (unsigned long long)level;
      ctr->eccentricity[i] = level;
    }
  }
  if (i == 0) {
    mirror[BM_TAIL] = (unsigned long long)__hip_atomic_exchange(&ctr->tail, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    mirror[BM_DEGSUM] = __hip_atomic_exchange(&ctr->degsum, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    mirror[BM_MAX_ROW] =
        (unsigned long long)__hip_atomic_exchange(&ctr->max_row, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    mirror[BM_READ] = __hip_atomic_load(&ctr->read, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ctr->big_n, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    stamp_handoff(mirror, sequence_slot, sequence);
  }
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

/**
 * @file truss_kernels.hxx
 * @brief K-truss decomposition (grx_truss): edge ids on the simple sorted copy, support by
 * triangle listing on its oriented copy, and a peel whose queue holds edges.
 *
 * The working copy S (sp, sj) is the simple graph under the caller's CSR, rows sorted by column.
 * Edge {u, v}, u < v, has the id of its entry (u, v) among the entries above the diagonal, in CSR
 * order; eid[] names it at both entries, eu[] / ev[] give its endpoints.
 *
 *   truss_cols_kernel       the kept (row, column) keys to their columns;
 *   truss_upper_kernel      entries of each row above the diagonal (the scan gives the first id of
 *                           every row);
 *   truss_edge_ids_kernel   eid at both entries (the lower one finds its mirror by binary search),
 *                           eu, ev.
 *
 * Support.  L is the degree-oriented copy of S as in tc_kernels.hxx: entry v of row u stays iff
 * rank(u) < rank(v), vertices ranked by (row length, id); a filter of sorted rows, so no sort.  leid[]
 * carries the edge id of every entry of L.  Every triangle {u, v, w}, rank u < v < w, is found once,
 * at u, by searching the entries w of out(v) in out(u), and adds one to its three edges: the slots
 * of (u, v) and (u, w) beside out(u), flushed by one atomic each, and the edge of the probed entry
 * (v, w) by an atomic of its own.  Integer adds: the sums do not depend on their order.  The rows
 * of L are binned by length and a row's probes are flattened over its workers:
 *   truss_orient_kernel<...>          the entries of L per row, then L and leid;
 *   truss_support_group_kernel<G>     rows of at most G entries, G lanes each (8 or 64), in LDS;
 *   truss_support_block_kernel<true>  a workgroup per row, out(u) staged in dynamic LDS (16 B per id);
 *   truss_support_block_kernel<false> rows longer than the staging capacity: searched in place, the
 *                                     prefix, base and counter slots in a global workspace at L's
 *                                     positions.
 *
 * Peel.  State per edge: support, truss (the answer) and stamp, the number of the generation that
 * holds the edge (TR_ALIVE: none yet).  At level k (floor f = k - 2) the seed scan queues the alive
 * edges with support <= f.  Working through generation G, edge e = {u, v} probes the shorter of its
 * rows into the longer; a common neighbour w gives e1 = {short, w}, e2 = {long, w}.  The triangle is
 * still there iff neither stamp is below G.  It is charged ONCE, by the smallest id among its edges
 * stamped G, to its edges NOT stamped G: atomic_sub, undone when the old value was at the floor; the
 * one decrement that reaches the floor stamps the edge G + 1 and appends it.  While G runs a stamp
 * only moves from TR_ALIVE to G + 1, both above G, so the three-way test (< G, == G, > G) does not
 * depend on timing, and neither does any final support or any generation's membership.
 *   truss_seed_kernel     the level's first generation and the smallest support above the floor;
 *   truss_wide_kernel     one generation, chunks of at most TR_BLOCK queued edges per workgroup;
 *   truss_narrow_kernel   ONE workgroup: generations while their probes are few, then the hand-off.
 * The queue (m slots, an edge is queued once) shares queue_counters_t, queue_sink_t, queue_flush,
 * narrow_generations and queue_publish with generation_queue.hxx; its append and its walk are its
 * own, because an item's length is min(row(u), row(v)) and not a row of the CSR.
 *
 *   truss_scatter_kernel  the answer to the caller's entries: binary search per entry, loops 0.
 */
#pragma once

#include <gunrock/hip/kernels/generation_queue.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int TR_BLOCK = 256;
constexpr int TR_NARROW_BLOCK = 1024;
constexpr int TR_NARROW_EDGES = 16384;  // default: generations with more probes go wide
constexpr int TR_SMALL = 8;             // rows of at most this many entries: 8 lanes each
constexpr int TR_WAVE = 64;             // ... one wavefront each
constexpr int TR_MEDIUM = 1024;         // ... one workgroup each, 16 KB of LDS
constexpr int TR_LDS_IDS = 8192;        // default staging capacity of the workgroup path (128 KB)
constexpr int TR_SLOT_BYTES = 16;       // per staged id: id, inclusive prefix, base, counter
constexpr int TR_CLASSES = 6;           // <2 entries (no triangle), group 8, group 64, medium, large, global
constexpr int TR_ALIVE = 0x7f7f7f7f;    // stamp of an edge no generation holds yet (a memset pattern)
constexpr unsigned TR_NONE = 0xffffffffu;

/// The working copy and its edge ids.
struct truss_graph_t {
  const int32_t *sp, *sj, *eid, *eu, *ev;
  int32_t n, m;  // vertices, edges (S has 2 m entries)
};
/// The peel's state, one word each per edge.
struct truss_state_t {
  int32_t *support, *stamp, *truss;
};

/// Position of w in the sorted id[0, d), or -1.
__device__ __forceinline__ int32_t truss_find(const int32_t* id, int32_t d, int32_t w) {
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

// ---------------------------------------------------------------------------
// the working copy
// ---------------------------------------------------------------------------

/// Kept entries of the sorted keys (at[e + 1] != at[e]) to their places.
__global__ void __launch_bounds__(TR_BLOCK)
    truss_cols_kernel(const unsigned long long* keys, const int* at, long long nnz, int32_t* sj) {
  for (long long e = blockIdx.x * (long long)TR_BLOCK + threadIdx.x; e < nnz; e += (long long)gridDim.x * TR_BLOCK)
    if (at[e + 1] != at[e])
      sj[at[e]] = (int32_t)(unsigned)keys[e];
}

/// upper[u] = entries of row u of S above the diagonal.
__global__ void __launch_bounds__(TR_BLOCK)
    truss_upper_kernel(const int32_t* sp, const int32_t* sj, int32_t n, int32_t* upper) {
  for (int64_t u = blockIdx.x * (int64_t)TR_BLOCK + threadIdx.x; u < n; u += (int64_t)gridDim.x * TR_BLOCK) {
    int32_t lo = sp[u];
    const int32_t end = sp[u + 1];
    int32_t hi = end;
    while (lo < hi) {  // first entry above u
      const int32_t mid = (lo + hi) >> 1;
      if (sj[mid] <= (int32_t)u)
        lo = mid + 1;
      else
        hi = mid;
    }
    upper[u] = end - lo;
  }
}

/// Edge ids of S's entries and the endpoints of every edge; ebase = exclusive scan of upper (n + 1).
/// A wavefront per row.
__global__ void __launch_bounds__(TR_BLOCK)
    truss_edge_ids_kernel(const int32_t* sp, const int32_t* sj, const int32_t* ebase, int32_t n, int32_t m,
                          int32_t* eid, int32_t* eu, int32_t* ev) {
  constexpr int WAVES = TR_BLOCK / wave_size;
  const int lane = lane_id();
  for (int64_t u = (int64_t)blockIdx.x * WAVES + threadIdx.x / wave_size; u < n; u += (int64_t)gridDim.x * WAVES) {
    const int32_t lo = sp[u], hi = sp[u + 1];
    const int32_t first = hi - (ebase[u + 1] - ebase[u]);  // the row's first entry above the diagonal
    for (int32_t p = lo + lane; p < hi; p += wave_size) {
      const int32_t v = sj[p];
      int32_t id = -1;
      if (p >= first) {
        id = ebase[u] + (p - first);
        if (id < m) {
          eu[id] = (int32_t)u;
          ev[id] = v;
        }
      } else {
        const int32_t vlo = sp[v], vhi = sp[v + 1];
        const int32_t q = truss_find(sj + vlo, vhi - vlo, (int32_t)u);
        const int32_t vfirst = vhi - (ebase[v + 1] - ebase[v]);
        if (q >= 0 && vlo + q >= vfirst)
          id = ebase[v] + (vlo + q - vfirst);
      }
      // a symmetric CSR (the call's gate) always finds its mirror; the clamp keeps every later index
      // inside [0, m) all the same
      eid[p] = id >= 0 && id < m ? id : 0;
    }
  }
}

// ---------------------------------------------------------------------------
// support
// ---------------------------------------------------------------------------

/// Size class of a row of d entries (bounds b[0..3] = group 8, group 64, medium, capacity).
__host__ __device__ __forceinline__ unsigned truss_class_of(int32_t d, const int32_t* b) {
  return d < 2 ? 0u : d <= b[0] ? 1u : d <= b[1] ? 2u : d <= b[2] ? 3u : d <= b[3] ? 4u : 5u;
}

/// starts[c] = first position of class c in the class-sorted keys (c = 0 .. TR_CLASSES).
__global__ void truss_class_starts_kernel(const unsigned* keys, int32_t n, int32_t* starts) {
  const int c = threadIdx.x;
  if (c > TR_CLASSES)
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

/// rank(u) < rank(v): vertices ordered by (row length of S, id).  du = row length of u.
__device__ __forceinline__ bool truss_before(const int32_t* sp, int32_t u, int32_t du, int32_t v) {
  const int32_t dv = sp[v + 1] - sp[v];
  return du < dv || (du == dv && u < v);
}

/// The oriented entries of each row of S (!WRITE: count[u]), or their columns and edge ids from
/// lap[u] on (WRITE).  S's rows are sorted and a filter keeps the order: L needs no sort.  A
/// wavefront per row.
template <bool WRITE>
__global__ void __launch_bounds__(TR_BLOCK)
    truss_orient_kernel(const int32_t* sp, const int32_t* sj, const int32_t* eid, int32_t n, int32_t* count,
                        const int32_t* lap, int32_t* laj, int32_t* leid) {
  constexpr int WAVES = TR_BLOCK / wave_size;
  const int lane = lane_id();
  for (int64_t u = (int64_t)blockIdx.x * WAVES + threadIdx.x / wave_size; u < n; u += (int64_t)gridDim.x * WAVES) {
    const int32_t lo = sp[u], hi = sp[u + 1], du = hi - lo;
    int32_t out = WRITE ? lap[u] : 0;
    for (int32_t e0 = lo; e0 < hi; e0 += wave_size) {
      const int32_t e = e0 + lane;
      bool keep = false;
      int32_t v = 0;
      if (e < hi) {
        v = sj[e];
        keep = truss_before(sp, (int32_t)u, du, v);
      }
      const unsigned long long mask = __ballot(keep);
      if (WRITE && keep) {
        const int32_t at = out + rank_in_mask(mask);
        laj[at] = v;
        leid[at] = eid[e];
      }
      out += __popcll(mask);
    }
    if (!WRITE && lane == 0)
      count[u] = out;
  }
}

/// Probes of the whole launch: one atomic per wavefront.
__device__ __forceinline__ void truss_flush_probes(unsigned long long probes, unsigned long long* total) {
  probes = wave_sum(probes);
  if (lane_id() == 0 && probes)
    atomicAdd(total, probes);
}

/// Rows of L with 2 .. G entries, G lanes each (TR_BLOCK / G rows per workgroup and batch).
template <int G>
__global__ void __launch_bounds__(TR_BLOCK)
    truss_support_group_kernel(const int32_t* lap, const int32_t* laj, const int32_t* leid, const int32_t* rows,
                               int32_t n_rows, int32_t* support, unsigned long long* total) {
  static_assert(G <= wave_size && TR_BLOCK % G == 0, "a row's lanes lie in one wavefront");
  constexpr int GROUPS = TR_BLOCK / G;
  __shared__ int32_t s_id[TR_BLOCK], s_pre[TR_BLOCK], s_base[TR_BLOCK], s_cnt[TR_BLOCK];
  const int l = threadIdx.x % G;
  const int first = threadIdx.x - l;
  int32_t* id = s_id + first;
  int32_t* pre = s_pre + first;
  int32_t* base = s_base + first;
  int32_t* cnt = s_cnt + first;
  unsigned long long probes = 0;
  // every group of the workgroup runs the same number of batches: the barriers are uniform
  for (int64_t r0 = (int64_t)blockIdx.x * GROUPS; r0 < n_rows; r0 += (int64_t)gridDim.x * GROUPS) {
    const int64_t r = r0 + threadIdx.x / G;
    int32_t d = 0, lo = 0;
    if (r < n_rows) {
      const int32_t u = rows[r];
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
    for (int32_t t = l; t < P; t += G) {
      const int32_t i = prefix_owner(pre, d, t);
      const int32_t pos = base[i] + t;  // entry (v_i, w) of L
      const int32_t j = truss_find(id, d, laj[pos]);
      if (j >= 0) {
        atomicAdd(&cnt[i], 1);
        atomicAdd(&cnt[j], 1);
        atomicAdd(&support[leid[pos]], 1);
      }
    }
    if (l == 0)
      probes += (unsigned long long)P;
    __syncthreads();
    // each lane flushes (and next batch rewrites) only its own slot
    if (l < d && cnt[l])
      atomicAdd(&support[leid[lo + l]], cnt[l]);
  }
  truss_flush_probes(probes, total);
}

/// One workgroup per row of L.  STAGED: out(u) and its slots in dynamic LDS (cap ids, 16 B each).
/// !STAGED: the row is searched in place and its slots are ws[0 | m | 2 m + L's positions].
template <bool STAGED>
__global__ void __launch_bounds__(TR_BLOCK)
    truss_support_block_kernel(const int32_t* lap, const int32_t* laj, const int32_t* leid, const int32_t* rows,
                               int32_t n_rows, int32_t cap, int32_t* ws, int64_t m, int32_t* support,
                               unsigned long long* total) {
  extern __shared__ int32_t s_dyn[];
  __shared__ int32_t s_wave[TR_BLOCK / wave_size + 1];
  const int tid = threadIdx.x;
  unsigned long long probes = 0;
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
    const int32_t per = (d + TR_BLOCK - 1) / TR_BLOCK;
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
    const int32_t offset = block_exclusive_sum<TR_BLOCK>(run, P, s_wave);
    for (int32_t i = c0; i < c1; ++i) {
      pre[i] += offset;
      base[i] -= offset;
    }
    __syncthreads();
    for (int32_t t = tid; t < P; t += TR_BLOCK) {
      const int32_t i = prefix_owner(pre, d, t);
      const int32_t pos = base[i] + t;  // entry (v_i, w) of L
      const int32_t j = truss_find(id, d, laj[pos]);
      if (j >= 0) {
        atomicAdd(&cnt[i], 1);
        atomicAdd(&cnt[j], 1);
        atomicAdd(&support[leid[pos]], 1);
      }
    }
    if (tid == 0)
      probes += (unsigned long long)P;
    __syncthreads();
    for (int32_t i = tid; i < d; i += TR_BLOCK) {
      // the global slots took atomics: read them where the atomics landed
      const int32_t c = STAGED ? cnt[i] : load_relaxed(&cnt[i]);
      if (c)
        atomicAdd(&support[leid[lo + i]], c);
    }
    __syncthreads();  // the next row restages the slots
  }
  truss_flush_probes(probes, total);
}

// ---------------------------------------------------------------------------
// peel
// ---------------------------------------------------------------------------

/// Device counters of one grx_truss call.
struct truss_counters_t : queue_counters_t {
  unsigned next_k;  // smallest remaining support above the level's floor, + 2 (TR_NONE: none)
  int gen;          // number of the pending generation
};
/// The mirror words the host reads per hand-off besides the queue's.
enum { TR_NEXT_K = GQ_WORDS, TR_GEN, TR_WORDS };

/// Probes of edge e when it leaves: the shorter of its two rows.
__device__ __forceinline__ int32_t truss_probes_of(const truss_graph_t& g, int32_t e) {
  const int32_t u = g.eu[e], v = g.ev[e];
  return min(g.sp[u + 1] - g.sp[u], g.sp[v + 1] - g.sp[v]);
}

/// queue_append for an item whose length the caller knows: append e for the lanes with `ready`;
/// every lane of the wavefront calls it.
template <bool NARROW>
__device__ __forceinline__ void truss_append(bool ready, int32_t e, int32_t len, const queue_sink_t& sink,
                                             unsigned long long& dsum) {
  const unsigned long long mask = __ballot(ready);
  if (mask) {
    const int first = __ffsll((long long)mask) - 1;
    int32_t base = 0;
    if (lane_id() == first)
      base = atomicAdd(sink.tail, __popcll(mask));
    base = __shfl(base, first, wave_size);
    if (ready) {
      const int32_t at = base + rank_in_mask(mask);
      if (at < sink.n) {  // an edge is queued once, so this holds; it guards the store all the same
        if (NARROW)       // read back by this workgroup in the next generation: past the L1
          store_relaxed(sink.queue + at, e);
        else
          sink.queue[at] = e;
      }
      dsum += (unsigned long long)len;
    }
  }
}

/// Flush a thread's running minimum: one atomic per wavefront.
__device__ __forceinline__ void truss_flush_min(unsigned mn, unsigned* next_k) {
  mn = wave_min(mn);
  if (lane_id() == 0 && mn != TR_NONE)
    atomicMin(next_k, mn);
}

/// The hand-off: ONE thread, last in its kernel.  When nothing is pending the level is over, and
/// the next level's seed scan starts next_k afresh.
__device__ __forceinline__ void truss_publish(truss_counters_t* ctr, unsigned long long* mirror, int sequence_slot,
                                              unsigned long long sequence, int head, int tail,
                                              unsigned long long degsum, unsigned next_k, int gen) {
  mirror[TR_NEXT_K] = next_k;
  mirror[TR_GEN] = (unsigned long long)gen;
  ctr->next_k = head == tail ? TR_NONE : next_k;
  ctr->gen = gen;
  queue_publish(ctr, mirror, sequence_slot, sequence, head, tail, degsum);
}

/// Level k: every alive edge with support <= k - 2 joins the pending generation; the smallest
/// support above the floor names the next level.
__global__ void __launch_bounds__(TR_BLOCK)
    truss_seed_kernel(truss_graph_t g, truss_state_t st, int32_t k, int32_t* queue, truss_counters_t* ctr) {
  const queue_sink_t sink{queue, g.m, &ctr->tail, &ctr->degsum};
  const int lane = lane_id();
  const int gen = ctr->gen;  // written by the hand-off before this kernel; constant here
  const int32_t floor = k - 2;
  unsigned mn = TR_NONE;
  unsigned long long dsum = 0;
  const int64_t stride = (int64_t)gridDim.x * TR_BLOCK;
  // whole wavefronts run every trip: the ballot of truss_append sees all 64 lanes
  for (int64_t e0 = blockIdx.x * (int64_t)TR_BLOCK + threadIdx.x - lane; e0 < g.m; e0 += stride) {
    const int64_t e = e0 + lane;
    bool leave = false;
    int32_t len = 0;
    if (e < g.m && st.stamp[e] == TR_ALIVE) {
      const int32_t s = st.support[e];
      if (s <= floor) {
        leave = true;
        st.stamp[e] = gen;
        len = truss_probes_of(g, (int32_t)e);
      } else {
        mn = min(mn, (unsigned)s + 2u);
      }
    }
    truss_append<false>(leave, (int32_t)e, len, sink, dsum);
  }
  truss_flush_min(mn, &ctr->next_k);
  queue_flush(dsum, &ctr->degsum);
}

/// Charge one triangle to its edge x, which generation `gen` does not hold: true for the one
/// decrement that brings x to the floor (x is then stamped gen + 1 and the caller appends it).
__device__ __forceinline__ bool truss_lower(const truss_state_t& st, int32_t x, int32_t floor, int gen, unsigned& mn) {
  // a support only falls towards the floor: a stale read errs towards the atomic
  if (load_relaxed(&st.support[x]) <= floor)
    return false;
  const int32_t old = atomicSub(&st.support[x], 1);
  if (old <= floor) {  // went under: x is at the floor and queued already
    atomicAdd(&st.support[x], 1);
    return false;
  }
  if (old - 1 == floor) {
    store_relaxed(&st.stamp[x], gen + 1);
    return true;
  }
  mn = min(mn, (unsigned)(old - 1) + 2u);
  return false;
}

/// Take queue[a, b) (b - a <= BLOCK), edges of generation `gen`, out at level k with the whole
/// workgroup: thread `tid` owns queue[a + tid], the probes of the chunk are flattened over the
/// threads in whole wavefronts.  Returns the probes.  Two barriers before the first append; ends
/// with a barrier.  `s_pre`, `s_base`, `s_e`, `s_long`: BLOCK words; `s_wave`: BLOCK / 64 + 1.
template <int BLOCK, bool NARROW>
__device__ __forceinline__ int32_t truss_peel_chunk(const truss_graph_t& g, const truss_state_t& st, int32_t a,
                                                    int32_t b, int32_t k, int gen, const queue_sink_t& sink,
                                                    int32_t* s_pre, int32_t* s_base, int32_t* s_e, int32_t* s_long,
                                                    int32_t* s_wave, unsigned& mn, unsigned long long& dsum) {
  const int tid = threadIdx.x;
  const int32_t floor = k - 2;
  int32_t lo = 0, d = 0;
  if (a + tid < b) {
    const int32_t e = NARROW ? load_relaxed(sink.queue + a + tid) : sink.queue[a + tid];
    const int32_t u = g.eu[e], v = g.ev[e];
    const int32_t ulo = g.sp[u], du = g.sp[u + 1] - ulo;
    const int32_t vlo = g.sp[v], dv = g.sp[v + 1] - vlo;
    const bool u_short = du <= dv;
    lo = u_short ? ulo : vlo;
    d = u_short ? du : dv;
    s_long[tid] = u_short ? v : u;
    s_e[tid] = e;
    st.truss[e] = k;
  }
  int32_t P = 0;
  const int32_t excl = block_exclusive_sum<BLOCK>(d, P, s_wave);
  s_pre[tid] = excl + d;
  s_base[tid] = lo - excl;
  __syncthreads();
  const int cnt = b - a;
  for (int32_t t0 = 0; t0 < P; t0 += BLOCK) {
    const int32_t t = t0 + tid;
    bool cross1 = false, cross2 = false;
    int32_t e1 = 0, e2 = 0;
    if (t < P) {
      const int o = prefix_owner(s_pre, cnt, t);
      const int32_t pos = s_base[o] + t;
      const int32_t L = s_long[o];
      const int32_t llo = g.sp[L];
      const int32_t q = truss_find(g.sj + llo, g.sp[L + 1] - llo, g.sj[pos]);
      if (q >= 0) {
        const int32_t e = s_e[o];
        e1 = g.eid[pos];
        e2 = g.eid[llo + q];
        const int s1 = load_relaxed(&st.stamp[e1]), s2 = load_relaxed(&st.stamp[e2]);
        if (s1 >= gen && s2 >= gen) {  // the triangle is still there
          const bool in1 = s1 == gen, in2 = s2 == gen;
          // charged once: by the smallest id among its edges of this generation
          if (!(in1 && e1 < e) && !(in2 && e2 < e)) {
            if (!in1)
              cross1 = truss_lower(st, e1, floor, gen, mn);
            if (!in2)
              cross2 = truss_lower(st, e2, floor, gen, mn);
          }
        }
      }
    }
    truss_append<NARROW>(cross1, e1, cross1 ? truss_probes_of(g, e1) : 0, sink, dsum);
    truss_append<NARROW>(cross2, e2, cross2 ? truss_probes_of(g, e2) : 0, sink, dsum);
  }
  __syncthreads();  // the next chunk rewrites the prefix
  return P;
}

__global__ void __launch_bounds__(TR_BLOCK)
    truss_wide_kernel(truss_graph_t g, truss_state_t st, int32_t* queue, int32_t head, int32_t tail, int32_t chunk,
                      int32_t k, int gen, truss_counters_t* ctr) {
  __shared__ int32_t s_pre[TR_BLOCK], s_base[TR_BLOCK], s_e[TR_BLOCK], s_long[TR_BLOCK],
      s_wave[TR_BLOCK / wave_size + 1];
  const queue_sink_t sink{queue, g.m, &ctr->tail, &ctr->degsum};
  unsigned mn = TR_NONE;
  unsigned long long dsum = 0, walked = 0;
  for (int64_t a = head + (int64_t)blockIdx.x * chunk; a < tail; a += (int64_t)gridDim.x * chunk) {
    const int32_t b = (int32_t)min((int64_t)tail, a + chunk);
    walked += (unsigned long long)truss_peel_chunk<TR_BLOCK, false>(g, st, (int32_t)a, b, k, gen, sink, s_pre, s_base,
                                                                    s_e, s_long, s_wave, mn, dsum);
  }
  truss_flush_min(mn, &ctr->next_k);
  queue_flush(dsum, &ctr->degsum);
  if (threadIdx.x == 0 && walked)
    atomicAdd(&ctr->edges, walked);
}

/// One workgroup: generations while their probes are at most `max_edges`, then the hand-off to the
/// host.  `advance`: 1 behind a wide kernel, which consumed the generation the counters name.
__global__ void __launch_bounds__(TR_NARROW_BLOCK)
    truss_narrow_kernel(truss_graph_t g, truss_state_t st, int32_t* queue, int32_t k, int advance,
                        unsigned long long max_edges, truss_counters_t* ctr, unsigned long long* mirror,
                        int sequence_slot, unsigned long long sequence) {
  __shared__ int32_t s_pre[TR_NARROW_BLOCK], s_base[TR_NARROW_BLOCK], s_e[TR_NARROW_BLOCK], s_long[TR_NARROW_BLOCK],
      s_wave[TR_NARROW_BLOCK / wave_size + 1];
  __shared__ int s_tail;
  __shared__ unsigned s_min;
  __shared__ unsigned long long s_dsum;
  if (threadIdx.x == 0)
    s_min = ctr->next_k;
  int gen = ctr->gen + advance;  // the same in every thread, here and after every generation
  unsigned mn = TR_NONE;
  const narrow_result_t r = narrow_generations(
      ctr, queue, g.m, INT32_MAX, max_edges, &s_tail, &s_dsum,
      [&](int32_t head, int32_t tail, const queue_sink_t& sink, unsigned long long& dsum) {
        unsigned long long walked = 0;
        for (int32_t a = head; a < tail; a += TR_NARROW_BLOCK)
          walked += (unsigned long long)truss_peel_chunk<TR_NARROW_BLOCK, true>(
              g, st, a, min(tail, a + TR_NARROW_BLOCK), k, gen, sink, s_pre, s_base, s_e, s_long, s_wave, mn, dsum);
        ++gen;
        return walked;
      });
  truss_flush_min(mn, &s_min);
  __syncthreads();
  if (threadIdx.x == 0) {
    ctr->edges += r.walked;  // no other kernel of the call runs beside this one
    truss_publish(ctr, mirror, sequence_slot, sequence, r.head, r.tail, r.degsum, s_min, gen);
  }
}

// ---------------------------------------------------------------------------
// the answer, to the caller's entries
// ---------------------------------------------------------------------------

/// out[p] = truss of the edge entry p of the caller's CSR names, 0 for a self loop.  A wavefront per row.
__global__ void __launch_bounds__(TR_BLOCK)
    truss_scatter_kernel(const int32_t* ap, const int32_t* aj, truss_graph_t g, const int32_t* truss, int32_t* out) {
  constexpr int WAVES = TR_BLOCK / wave_size;
  const int lane = lane_id();
  for (int64_t u = (int64_t)blockIdx.x * WAVES + threadIdx.x / wave_size; u < g.n; u += (int64_t)gridDim.x * WAVES) {
    const int32_t lo = ap[u], hi = ap[u + 1];
    const int32_t slo = g.sp[u], sd = g.sp[u + 1] - slo;
    for (int32_t p = lo + lane; p < hi; p += wave_size) {
      const int32_t v = aj[p];
      int32_t value = 0;
      if (v != (int32_t)u) {
        const int32_t q = truss_find(g.sj + slo, sd, v);
        if (q >= 0)
          value = truss[g.eid[slo + q]];
      }
      out[p] = value;
    }
  }
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

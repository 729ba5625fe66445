/**
 * @file scc_kernels.hxx
 * @brief Strongly connected components (grx_scc): forward-backward with trimming, all regions at
 * once, on the generation queue.
 *
 * A REGION is a set of unfinished vertices known to be a union of whole SCCs; at the start one
 * region holds everything.  An entry (u, v) of either array is ALIVE when u != v, both ends are
 * unfinished and both lie in the same region.  Two facts carry the correctness:
 *
 *   Trim.  An unfinished vertex with no alive out-entry or no alive in-entry is an SCC of one: a
 *   cycle through it would need one of each, inside its region.
 *   Forward-backward.  For a pivot p of region R let FW and BW be the vertices p reaches, and is
 *   reached from, along alive entries.  FW n BW is p's SCC.  Every other SCC of R lies wholly in one
 *   of FW \ BW, BW \ FW and R \ (FW u BW): if one member of an SCC is in FW (BW), all are.  Those
 *   three sets are the regions of the next round.
 *
 * State: st[V] (64-bit: bit 0 finished, bit 1 in FW, bit 2 in BW, bits 3..4 the region's class,
 * bits 32..63 its owner; st >> 3 names the region), out_cnt[V] / in_cnt[V] (alive out- / in-entries,
 * repeats counted each time), label[V] (the answer), queue[V] and table[3 V + 1] (64-bit: the
 * largest key of every region).  A region is (owner, class): the start region is (0, 0) in slot 0;
 * the remainders of the region whose pivot was p are (p, 1) = FW \ BW, (p, 2) = BW \ FW and (p, 3) =
 * the rest, in slot 3 p + class, a size_t.  A vertex is a pivot once (its round finishes it), so
 * every name is new, no slot is written in two rounds and the table is cleared once per call.
 * The pivot of a region is read back from its slot: the key's low word is fmix32(p), a bijection.
 *
 *   scc_count_kernel       all rows of both arrays, a chunk of SCC_BLOCK consecutive vertices per
 *                          workgroup (flat_walk): out_cnt / in_cnt of the unfinished vertices.  Rows
 *                          above `big_row` are cut into segments (push_big_segments) ...
 *   scc_count_big_kernel   ... counted a workgroup per segment.
 *   scc_trim_seed_kernel   every unfinished vertex with a zero count is claimed and queued.
 *   scc_wide_kernel<true>  one trim generation, a chunk of at most SCC_BLOCK queued vertices per
 *                          workgroup: label = own id; the out-rows lower in_cnt of the alive targets,
 *                          the in-rows out_cnt of the alive sources (two queue_walks, the second over
 *                          the in-edge arrays).  The decrement that returns 1 claims the vertex
 *                          (atomic_or of the finished bit: two counts can reach 0, one claim wins)
 *                          and appends it.  Rows longer than `big_row` go to two lists ...
 *   scc_big_kernel         ... and are walked by the whole grid.
 *   scc_pivot_max_kernel   key(v) = (min(out_cnt * in_cnt, 2^32 - 1) << 32) | fmix32(v) of every
 *                          unfinished vertex into its region's slot by a 64-bit atomic_max.
 *   scc_pivot_seed_kernel  the vertex that finds its own key there is the pivot: it enters FW and
 *                          BW, label = own id, and it is queued: the seed generation.
 *   scc_wide_kernel<false> one reach generation over the out-rows (FW) or the in-rows (BW): an alive
 *                          entry's other end is claimed by atomic_or of the bit, behind a plain
 *                          pre-test (a stale read only errs towards the atomic), and the claimer
 *                          appends it: queued at most once per reach, so V slots hold.
 *   scc_rewind_kernel      the queue is the seed generation again, for the backward reach.
 *   scc_narrow_kernel      ONE workgroup that runs consecutive small generations (trim or reach) by
 *                          itself, then hands the counters to the host: it ends every batch.
 *   scc_min_kernel         every member of FW n BW: atomic_min of its id into the pivot's label.
 *   scc_finish_kernel      FW n BW takes that label and is finished; the others take the name of
 *                          their remainder, with FW and BW cleared.
 *
 * No kernel waits on another workgroup.  A claimed vertex is never claimed again, and the counts of
 * an unfinished vertex are exact once a phase is over: every finished neighbour of its region
 * lowered them once per entry, when its own row was walked.  st changes by atomics only (the
 * finish kernel's store is an atomic store of the vertex's own word); the narrow workgroup loads st
 * and the queue past the L1.  Every queue store is guarded by `at < n` (queue_append).
 *
 * Hooks (capi_scc.hip, through env_or): GRX_SCC_BIG_ROW (default 4096), GRX_SCC_NARROW_EDGES
 * (default 16384; 0 = never narrow), GRX_SCC_TRIM (default 1; 0 = no trimming, singletons are
 * found as pivots).
 */
#pragma once

#include <gunrock/hip/kernels/generation_queue.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int SCC_BLOCK = 256;
constexpr int SCC_NARROW_BLOCK = 1024;   // also the narrow kernel's capacity in vertices
constexpr int SCC_NARROW_EDGES = 16384;  // default: generations with more entries go wide
constexpr int SCC_BIG_ROW = 4096;        // default: longer rows are walked by the whole grid
constexpr int SCC_BIG_SEGMENT = 4096;    // the counting pass cuts them into segments of this many

using scc_state_t = unsigned long long;
constexpr scc_state_t SCC_DONE = 1, SCC_FW = 2, SCC_BW = 4;
constexpr int SCC_REGION_SHIFT = 3;  // st >> 3: (owner << 29) | class, the region's name

/// One direction of the graph: the CSR's arrays or the in-edge arrays.
struct scc_rows_t {
  const int32_t* ap;
  const int32_t* aj;
};

/// Device counters of one grx_scc call.
struct scc_counters_t : queue_counters_t {
  int big_in_n;                 // in-rows on their big list (big_n: the out-rows, or a reach's rows)
  int seg_n;                    // segments of the counting pass
  int seeds, pad;               // pivots of the round
  unsigned long long seed_in;   // entries of their in-rows
  unsigned long long finished;  // members of FW n BW finished so far
};
/// The mirror words the host reads per hand-off besides the queue's.
enum { SC_SEEDS = GQ_WORDS, SC_SEED_IN, SC_FINISHED, SC_WORDS };

/// fmix32's inverse: the pivot of a region from the low word of its slot.
__host__ __device__ __forceinline__ unsigned scc_unmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x7ed1b41du;
  h ^= (h >> 13) ^ (h >> 26);
  h *= 0xa5cb9243u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ std::size_t scc_slot(scc_state_t sv) {
  return (std::size_t)3 * (std::size_t)(sv >> 32) + (std::size_t)((sv >> SCC_REGION_SHIFT) & 3);
}

__device__ __forceinline__ unsigned long long scc_key(const int32_t* out_cnt, const int32_t* in_cnt, int32_t v) {
  const unsigned long long prod = (unsigned long long)(unsigned)out_cnt[v] * (unsigned long long)(unsigned)in_cnt[v];
  return (min(prod, 0xffffffffull) << 32) | fmix32((unsigned)v);
}

__device__ __forceinline__ int32_t scc_pivot_of(const unsigned long long* table, scc_state_t sv) {
  return (int32_t)scc_unmix32((unsigned)table[scc_slot(sv)]);
}

template <bool NARROW>
__device__ __forceinline__ scc_state_t scc_state(const scc_state_t* st, int32_t v) {
  return NARROW ? load_relaxed(st + v) : st[v];
}

/// One entry w of the row of queued vertex u in region `reg` (`active` lanes hold one); every lane
/// of the wavefront calls it.  TRIM: u left, so w has one alive entry less in `cnt`; whoever takes it
/// to 0 claims w.  Otherwise a reach: w is claimed for `bit`.  The claimer appends w.
template <bool NARROW, bool TRIM>
__device__ __forceinline__ void scc_relax(bool active, int32_t w, int32_t u, scc_state_t reg, scc_state_t bit,
                                          int32_t* cnt, scc_state_t* st, const int32_t* ap, const int32_t* other_ap,
                                          const queue_sink_t& sink, unsigned long long& dsum) {
  bool claim = false;
  if (active && w != u) {
    const scc_state_t sw = scc_state<NARROW>(st, w);
    if (!(sw & (SCC_DONE | bit)) && (sw >> SCC_REGION_SHIFT) == reg) {
      if (TRIM) {
        if (atomicSub(&cnt[w], 1) == 1)
          claim = !(atomicOr(&st[w], SCC_DONE) & SCC_DONE);
      } else {
        claim = !(atomicOr(&st[w], bit) & bit);
      }
    }
  }
  queue_append<NARROW>(claim, w, ap, sink, dsum);
  if (TRIM && claim)  // a trimmed vertex walks both of its rows
    dsum += (unsigned long long)(other_ap[w + 1] - other_ap[w]);
}

/// LDS of a workgroup that works through chunks of BLOCK queued vertices.
template <int BLOCK>
struct scc_chunk_lds_t {
  scc_state_t reg[BLOCK];  // the owners' regions
  int32_t pre[BLOCK], base[BLOCK], vert[BLOCK];
  int32_t wave[BLOCK / wave_size + 1];
};

/// What a generation's kernels work on.  TRIM: a = out-rows, b = in-rows; a reach: a = its rows.
struct scc_pass_t {
  scc_rows_t a, b;
  scc_state_t bit;
  scc_state_t* st;
  int32_t *out_cnt, *in_cnt, *label;
  int32_t big_row;
  int32_t *big_a, *big_b;
};

/// Work through queue[a, b) (b - a <= BLOCK) with the whole workgroup.  Returns the entries walked.
/// Ends with a barrier.
template <int BLOCK, bool NARROW, bool TRIM>
__device__ __forceinline__ int32_t scc_chunk(const scc_pass_t& p, int32_t a, int32_t b, scc_counters_t* ctr,
                                             const queue_sink_t& sink, scc_chunk_lds_t<BLOCK>& s,
                                             unsigned long long& dsum) {
  const int tid = threadIdx.x;
  int32_t P = queue_walk<BLOCK, NARROW>(
      p.a.ap, sink.queue, a, b, s.pre, s.base, s.wave,
      [&](int32_t u, int32_t, int32_t& d) {
        if (TRIM)
          p.label[u] = u;
        s.vert[tid] = u;
        s.reg[tid] = scc_state<NARROW>(p.st, u) >> SCC_REGION_SHIFT;
        if (!NARROW)
          queue_divert_big(u, d, p.big_row, p.big_a, &ctr->big_n);
      },
      [&](bool live, int o, int32_t e) {
        scc_relax<NARROW, TRIM>(live, live ? p.a.aj[e] : 0, live ? s.vert[o] : 0, live ? s.reg[o] : 0, p.bit,
                                p.in_cnt, p.st, p.a.ap, p.b.ap, sink, dsum);
      });
  if (TRIM)
    P += queue_walk<BLOCK, NARROW>(
        p.b.ap, sink.queue, a, b, s.pre, s.base, s.wave,
        [&](int32_t u, int32_t, int32_t& d) {
          if (!NARROW)
            queue_divert_big(u, d, p.big_row, p.big_b, &ctr->big_in_n);
        },
        [&](bool live, int o, int32_t e) {
          scc_relax<NARROW, true>(live, live ? p.b.aj[e] : 0, live ? s.vert[o] : 0, live ? s.reg[o] : 0, 0,
                                  p.out_cnt, p.st, p.a.ap, p.b.ap, sink, dsum);
        });
  return P;
}

__global__ void __launch_bounds__(SCC_BLOCK)
    scc_count_kernel(scc_rows_t out, scc_rows_t in, const scc_state_t* st, int32_t n, int32_t big_row,
                     int32_t* out_cnt, int32_t* in_cnt, int2* seg, scc_counters_t* ctr) {
  __shared__ int32_t s_pre[SCC_BLOCK], s_base[SCC_BLOCK], s_wave[SCC_BLOCK / wave_size + 1];
  __shared__ int32_t s_count[SCC_BLOCK];
  __shared__ scc_state_t s_reg[SCC_BLOCK];
  const int tid = threadIdx.x;
  unsigned long long walked = 0;
  unsigned mxrow = 0;
  for (int64_t v0 = (int64_t)blockIdx.x * SCC_BLOCK; v0 < n; v0 += (int64_t)gridDim.x * SCC_BLOCK) {
    const int64_t v = v0 + tid;
    const scc_state_t sv = v < n ? st[v] : SCC_DONE;
    const bool unfinished = !(sv & SCC_DONE);
    s_reg[tid] = sv >> SCC_REGION_SHIFT;
    for (int dir = 0; dir < 2; ++dir) {
      const scc_rows_t rows = dir ? in : out;
      int32_t lo = 0, d = 0;
      if (unfinished) {
        lo = rows.ap[v];
        d = max(rows.ap[v + 1] - lo, 0);
        mxrow = max(mxrow, (unsigned)d);
        if (d > big_row) {  // an in-row is listed under ~v
          push_big_segments<SCC_BIG_SEGMENT>(&ctr->seg_n, seg, dir ? ~(int32_t)v : (int32_t)v, d);
          walked += (unsigned long long)d;
          d = 0;
        }
      }
      s_count[tid] = 0;
      const int32_t P = flat_walk<SCC_BLOCK>(d, lo, s_pre, s_base, s_wave, [&](int o, int32_t e) {
        const int32_t w = rows.aj[e];
        if (w != (int32_t)v0 + o) {
          const scc_state_t sw = st[w];
          if (!(sw & SCC_DONE) && (sw >> SCC_REGION_SHIFT) == s_reg[o])
            atomicAdd(&s_count[o], 1);
        }
      });
      walked += (unsigned long long)(tid == 0 ? P : 0);
      // s_count is complete behind flat_walk's trailing barrier (P == 0: nobody wrote it)
      if (unfinished)
        (dir ? in_cnt : out_cnt)[v] = s_count[tid];  // a big row: 0, its segments add to it in the next kernel
    }
  }
  walked = wave_sum(walked);
  mxrow = wave_max(mxrow);
  if (lane_id() == 0) {
    if (walked)
      atomicAdd(&ctr->edges, walked);
    if (mxrow)
      atomicMax(&ctr->max_row, mxrow);
  }
}

/// The segments of the long rows, one workgroup each: the count of their vertex += alive entries.
__global__ void __launch_bounds__(SCC_BLOCK)
    scc_count_big_kernel(scc_rows_t out, scc_rows_t in, const scc_state_t* st, int32_t* out_cnt, int32_t* in_cnt,
                         const int2* seg, const scc_counters_t* ctr) {
  __shared__ int32_t s_sum[SCC_BLOCK / wave_size];
  const int32_t items = ctr->seg_n;  // written by the count kernel before this one; constant here
  for (int32_t i = blockIdx.x; i < items; i += gridDim.x) {
    const int2 item = seg[i];  // {vertex (~vertex: its in-row), segment of the row}
    const bool inward = item.x < 0;
    const int32_t v = inward ? ~item.x : item.x;
    const scc_rows_t rows = inward ? in : out;
    const scc_state_t reg = st[v] >> SCC_REGION_SHIFT;
    const int64_t lo = (int64_t)rows.ap[v] + (int64_t)item.y * SCC_BIG_SEGMENT;
    const int64_t hi = min((int64_t)rows.ap[v + 1], lo + SCC_BIG_SEGMENT);
    int32_t count = 0;
    for (int64_t e = lo + threadIdx.x; e < hi; e += SCC_BLOCK) {
      const int32_t w = rows.aj[e];
      if (w != v) {
        const scc_state_t sw = st[w];
        count += !(sw & SCC_DONE) && (sw >> SCC_REGION_SHIFT) == reg;
      }
    }
    count = block_sum<SCC_BLOCK>(count, s_sum);
    if (threadIdx.x == 0 && count)
      atomicAdd(&(inward ? in_cnt : out_cnt)[v], count);
    __syncthreads();  // the next item rewrites s_sum
  }
}

/// The first trim generation: the unfinished vertices with a zero count.
__global__ void __launch_bounds__(SCC_BLOCK)
    scc_trim_seed_kernel(const int32_t* out_ap, const int32_t* in_ap, scc_state_t* st, const int32_t* out_cnt,
                         const int32_t* in_cnt, int32_t n, int32_t* queue, scc_counters_t* ctr) {
  const queue_sink_t sink{queue, n, &ctr->tail, &ctr->degsum};
  const int lane = lane_id();
  unsigned long long dsum = 0;
  const int64_t stride = (int64_t)gridDim.x * SCC_BLOCK;
  // whole wavefronts run every trip: the ballot of queue_append sees all 64 lanes
  for (int64_t v0 = blockIdx.x * (int64_t)SCC_BLOCK + threadIdx.x - lane; v0 < n; v0 += stride) {
    const int64_t v = v0 + lane;
    bool leave = false;
    if (v < n && !(st[v] & SCC_DONE) && (out_cnt[v] == 0 || in_cnt[v] == 0)) {
      leave = !(atomicOr(&st[v], SCC_DONE) & SCC_DONE);
      if (leave)
        dsum += (unsigned long long)(in_ap[v + 1] - in_ap[v]);
    }
    queue_append<false>(leave, (int32_t)v, out_ap, sink, dsum);
  }
  queue_flush(dsum, &ctr->degsum);
}

__global__ void __launch_bounds__(SCC_BLOCK)
    scc_pivot_max_kernel(const scc_state_t* st, const int32_t* out_cnt, const int32_t* in_cnt, int32_t n,
                         unsigned long long* table) {
  for (int64_t v = blockIdx.x * (int64_t)SCC_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * SCC_BLOCK) {
    const scc_state_t sv = st[v];
    if (sv & SCC_DONE)
      continue;
    const unsigned long long key = scc_key(out_cnt, in_cnt, (int32_t)v);
    unsigned long long* slot = table + scc_slot(sv);
    if (*slot < key)  // a stale read is smaller: it only errs towards the atomic
      atomicMax(slot, key);
  }
}

/// The pivots: in FW and BW, their own label until a smaller member is found, and the seed generation.
__global__ void __launch_bounds__(SCC_BLOCK)
    scc_pivot_seed_kernel(const int32_t* out_ap, const int32_t* in_ap, scc_state_t* st, const int32_t* out_cnt,
                          const int32_t* in_cnt, int32_t n, const unsigned long long* table, int32_t* label,
                          int32_t* queue, scc_counters_t* ctr) {
  const queue_sink_t sink{queue, n, &ctr->tail, &ctr->degsum};
  const int lane = lane_id();
  unsigned long long dsum = 0, in_sum = 0;
  int seeds = 0;
  const int64_t stride = (int64_t)gridDim.x * SCC_BLOCK;
  // whole wavefronts run every trip: the ballot of queue_append sees all 64 lanes
  for (int64_t v0 = blockIdx.x * (int64_t)SCC_BLOCK + threadIdx.x - lane; v0 < n; v0 += stride) {
    const int64_t v = v0 + lane;
    bool pivot = false;
    if (v < n) {
      const scc_state_t sv = st[v];
      pivot = !(sv & SCC_DONE) && table[scc_slot(sv)] == scc_key(out_cnt, in_cnt, (int32_t)v);
      if (pivot) {
        atomicOr(&st[v], SCC_FW | SCC_BW);
        label[v] = (int32_t)v;
        in_sum += (unsigned long long)(in_ap[v + 1] - in_ap[v]);
        ++seeds;
      }
    }
    queue_append<false>(pivot, (int32_t)v, out_ap, sink, dsum);
  }
  queue_flush(dsum, &ctr->degsum);
  queue_flush(in_sum, &ctr->seed_in);
  seeds = wave_sum(seeds);
  if (lane == 0 && seeds)
    atomicAdd(&ctr->seeds, seeds);
}

/// The backward reach starts from the seed generation, which still heads the queue.
__global__ void scc_rewind_kernel(scc_counters_t* ctr, int seeds, unsigned long long seed_in) {
  if (threadIdx.x == 0) {
    ctr->head = 0;
    ctr->tail = seeds;
    ctr->degsum = seed_in;
  }
}

template <bool TRIM>
__global__ void __launch_bounds__(SCC_BLOCK)
    scc_wide_kernel(scc_pass_t p, int32_t* queue, int32_t n, int32_t head, int32_t tail, int32_t chunk,
                    scc_counters_t* ctr) {
  __shared__ scc_chunk_lds_t<SCC_BLOCK> s;
  const queue_sink_t sink{queue, n, &ctr->tail, &ctr->degsum};
  unsigned long long dsum = 0, walked = 0;
  for (int64_t a = head + (int64_t)blockIdx.x * chunk; a < tail; a += (int64_t)gridDim.x * chunk) {
    const int32_t b = (int32_t)min((int64_t)tail, a + chunk);
    walked += (unsigned long long)scc_chunk<SCC_BLOCK, false, TRIM>(p, (int32_t)a, b, ctr, sink, s, dsum);
  }
  queue_flush(dsum, &ctr->degsum);
  if (threadIdx.x == 0 && walked)
    atomicAdd(&ctr->edges, walked);
}

/// `rows` rows of `list`, each spread over the whole grid.
template <bool TRIM>
__device__ __forceinline__ void scc_big_rows(const scc_pass_t& p, scc_rows_t rows, const int32_t* list, int32_t count,
                                             int32_t* cnt, const queue_sink_t& sink, unsigned long long& dsum,
                                             unsigned long long& walked) {
  for (int32_t r = 0; r < count; ++r) {
    const int32_t u = list[r];
    const scc_state_t reg = p.st[u] >> SCC_REGION_SHIFT;
    const int32_t lo = rows.ap[u], hi = rows.ap[u + 1];
    walked += (unsigned long long)(hi - lo);
    for (int64_t e0 = lo + (int64_t)blockIdx.x * SCC_BLOCK; e0 < hi; e0 += (int64_t)gridDim.x * SCC_BLOCK) {
      const int64_t e = e0 + threadIdx.x;
      scc_relax<false, TRIM>(e < hi, e < hi ? rows.aj[e] : 0, u, reg, p.bit, cnt, p.st, p.a.ap, p.b.ap, sink, dsum);
    }
  }
}

/// The rows on the big lists: a trim generation's out-rows and in-rows, or a reach's rows.
template <bool TRIM>
__global__ void __launch_bounds__(SCC_BLOCK) scc_big_kernel(scc_pass_t p, int32_t* queue, int32_t n, scc_counters_t* ctr) {
  const queue_sink_t sink{queue, n, &ctr->tail, &ctr->degsum};
  // written by the wide kernel before this one; constant here
  const int32_t rows_a = ctr->big_n, rows_b = TRIM ? ctr->big_in_n : 0;
  unsigned long long dsum = 0, walked = 0;
  scc_big_rows<TRIM>(p, p.a, p.big_a, rows_a, p.in_cnt, sink, dsum, walked);
  if (TRIM)
    scc_big_rows<true>(p, p.b, p.big_b, rows_b, p.out_cnt, sink, dsum, walked);
  queue_flush(dsum, &ctr->degsum);
  if (blockIdx.x == 0 && threadIdx.x == 0 && walked)
    atomicAdd(&ctr->edges, walked);
}

/// The hand-off: ONE thread, last in its kernel.  The round's pivots are read by the host once and
/// counted afresh in the next round; the lists of the next batch start empty.
__device__ __forceinline__ void scc_publish(scc_counters_t* ctr, unsigned long long* mirror, int sequence_slot,
                                            unsigned long long sequence, int head, int tail,
                                            unsigned long long degsum) {
  mirror[SC_SEEDS] = (unsigned long long)ctr->seeds;
  mirror[SC_SEED_IN] = ctr->seed_in;
  mirror[SC_FINISHED] = ctr->finished;
  ctr->seeds = 0;
  ctr->seed_in = 0;
  ctr->seg_n = 0;
  ctr->big_in_n = 0;
  queue_publish(ctr, mirror, sequence_slot, sequence, head, tail, degsum);
}

/// One workgroup: generations while they are small, then the hand-off to the host.
template <bool TRIM>
__global__ void __launch_bounds__(SCC_NARROW_BLOCK)
    scc_narrow_kernel(scc_pass_t p, int32_t* queue, int32_t n, int32_t max_vertices, unsigned long long max_edges,
                      scc_counters_t* ctr, unsigned long long* mirror, int sequence_slot,
                      unsigned long long sequence) {
  __shared__ scc_chunk_lds_t<SCC_NARROW_BLOCK> s;
  __shared__ int s_tail;
  __shared__ unsigned long long s_dsum;
  const narrow_result_t r = narrow_generations(
      ctr, queue, n, max_vertices, max_edges, &s_tail, &s_dsum,
      [&](int32_t head, int32_t tail, const queue_sink_t& sink, unsigned long long& dsum) {
        return scc_chunk<SCC_NARROW_BLOCK, true, TRIM>(p, head, tail, ctr, sink, s, dsum);
      });
  if (threadIdx.x == 0) {
    ctr->edges += r.walked;  // no other kernel of the call runs beside this one
    scc_publish(ctr, mirror, sequence_slot, sequence, r.head, r.tail, r.degsum);
  }
}

/// The label of FW n BW is the minimum id of its members, gathered in the pivot's slot.
__global__ void __launch_bounds__(SCC_BLOCK)
    scc_min_kernel(const scc_state_t* st, int32_t n, const unsigned long long* table, int32_t* label) {
  for (int64_t v = blockIdx.x * (int64_t)SCC_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * SCC_BLOCK) {
    const scc_state_t sv = st[v];
    if ((sv & (SCC_DONE | SCC_FW | SCC_BW)) != (SCC_FW | SCC_BW))
      continue;
    const int32_t p = scc_pivot_of(table, sv);
    if ((int32_t)v < label[p])  // a stale read is larger: it only errs towards the atomic
      atomicMin(&label[p], (int32_t)v);
  }
}

/// FW n BW is finished; the rest of every region takes the name of its remainder.  A vertex writes
/// its own word only and reads nobody else's.
__global__ void __launch_bounds__(SCC_BLOCK)
    scc_finish_kernel(scc_state_t* st, int32_t n, const unsigned long long* table, int32_t* label,
                      scc_counters_t* ctr) {
  unsigned long long finished = 0;
  for (int64_t v = blockIdx.x * (int64_t)SCC_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * SCC_BLOCK) {
    const scc_state_t sv = st[v];
    if (sv & SCC_DONE)
      continue;
    const int32_t p = scc_pivot_of(table, sv);
    const bool fw = sv & SCC_FW, bw = sv & SCC_BW;
    if (fw && bw) {
      if ((int32_t)v != p)  // nobody writes label[p] here
        label[v] = label[p];
      store_relaxed(st + v, sv | SCC_DONE);
      ++finished;
    } else {
      const scc_state_t cls = fw ? 1 : bw ? 2 : 3;
      store_relaxed(st + v, ((scc_state_t)(unsigned)p << 32) | (cls << SCC_REGION_SHIFT));
    }
  }
  finished = wave_sum(finished);
  if (lane_id() == 0 && finished)
    atomicAdd(&ctr->finished, finished);
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

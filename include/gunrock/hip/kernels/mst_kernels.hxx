/**
 * @file mst_kernels.hxx
 * @brief Minimum spanning forest (grx_mst): Boruvka rounds on a flat component array, every row
 * entry an undirected candidate ordered by the 64-bit key (ordered_bits(weight) << 32) | position.
 *
 * State: comp[V] (the root of each vertex's component, FLAT between rounds: comp[comp[v]] ==
 * comp[v]), best[V] (the smallest key that leaves each component, MST_NONE when none), link[V] (where
 * each root of the round hooks; read at roots only), done[V] (row flags: every entry of the row is
 * inside one component, which stays true for ever) and a bitmap over entry positions (the chosen).
 *
 *   mst_init_kernel     comp[v] = v, best[v] = MST_NONE, done[v] = 0.
 *   mst_search_kernel   a chunk of MST_BLOCK consecutive rows per workgroup, their entries flattened
 *                       over the workgroup's threads (flat_walk, row_walk.hxx).  An entry whose ends
 *                       lie in different components offers its key to BOTH (pre-tested 64-bit atomic
 *                       min): the order includes the position, so the entry (v, u) stored in row v
 *                       is another candidate than (u, v).  A row none of whose entries left its
 *                       component is flagged and costs one byte load from then on.  Rows above
 *                       `big_row` entries go to a list in segments of MST_BIG_SEGMENT ...
 *   mst_big_kernel      ... a workgroup per segment; the row's own side is reduced per wave first.
 *   mst_hook_kernel     every root r with a key hooks under the component at the other end of its
 *                       entry: link[r] = other, and the entry's bit is set.  The strict order allows
 *                       no cycle but two roots that picked the SAME entry: the smaller root id stays
 *                       root (link[r] = r) and the other one records the entry, once.
 *   mst_jump_kernel     link[r] = link[link[r]] over the round's roots; pass j leaves at once when
 *                       pass j - 1 changed nothing (a word of the counters), so the host can enqueue
 *                       ceil(log2(bound on the tree depth)) of them blind.
 *   mst_flatten_kernel  comp[v] = link[comp[v]], best[v] = MST_NONE.
 *   mst_publish_kernel  copies the counters to the host's mirror, clears the round's, stamps the
 *                       hand-off.
 *   after the loop: mst_minid_* (labels: the smallest vertex id of each component), mst_tile_count /
 *   mst_tile_scan / mst_emit (the bitmap to ascending positions and per-tile float64 sums) and
 *   mst_sum_kernel (the tile sums in a fixed tree: no float atomics anywhere).
 *
 * comp[] and best[] do not change while a kernel that reads them plainly runs (search reads comp and
 * changes best by atomics only; hook reads both and writes link and the bitmap; flatten reads link
 * and writes each thread's own comp word).  link[] IS read while other CUs write it (mst_jump_kernel):
 * those are relaxed agent-scope atomic loads and stores (load_relaxed / store_relaxed).
 */
#pragma once

#include <gunrock/hip/kernels/row_walk.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int MST_BLOCK = 256;
constexpr int MST_BIG_ROW = 4096;      // default: rows with more entries go to the big list ...
constexpr int MST_BIG_SEGMENT = 4096;  // ... in segments of this many entries, a workgroup each
constexpr int MST_SCAN_BLOCK = 1024;   // the single workgroup of the scan and of the last sum
constexpr int MST_MAX_JUMPS = 32;      // pointer-jumping passes a round can enqueue
constexpr unsigned long long MST_NONE = ~0ull;

/// Device counters of one grx_mst call.
struct mst_counters_t {
  unsigned long long edges;   // row entries the search kernels read, all rounds
  unsigned long long hooked;  // roots that hooked in this round
  unsigned long long count;   // chosen entries (the scan's total)
  double weight;              // their weights' sum
  int big_n;                  // segments on this round's big list
  int changed[MST_MAX_JUMPS];  // jump pass j of this round changed a word
};
/// What the host reads at a hand-off (words of the pinned mirror).
enum { MST_EDGES = 0, MST_HOOKED, MST_COUNT, MST_WEIGHT, MST_WORDS };

/// Monotone map of a float onto uint32: a < b as floats  =>  bits(a) < bits(b); -0 maps below +0.
__host__ __device__ __forceinline__ uint32_t mst_ordered_bits(float w) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t b = __float_as_uint(w);
#else
  uint32_t b;
  __builtin_memcpy(&b, &w, 4);
#endif
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ unsigned long long mst_key(float w, int32_t e) {
  return ((unsigned long long)mst_ordered_bits(w) << 32) | (unsigned long long)(uint32_t)e;
}

/// Pre-tested atomic min: most offers lose, and a loser costs one L2-served load (util/math.hxx).
__device__ __forceinline__ void mst_min(unsigned long long* p, unsigned long long key) {
  if (load_relaxed(p) > key)
    atomicMin(p, key);
}

/// Largest u in [0, n) with ap[u] <= e: the row that holds entry position e (0 <= e < ap[n]).
__device__ __forceinline__ int32_t mst_row_of(const int32_t* ap, int32_t n, int32_t e) {
  int32_t lo = 0, hi = n;  // answer in [lo, hi)
  while (hi - lo > 1) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (ap[mid] <= e)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(MST_BLOCK)
    mst_init_kernel(int32_t* comp, unsigned long long* best, unsigned char* done, int32_t n) {
  for (int64_t v = blockIdx.x * (int64_t)MST_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * MST_BLOCK) {
    comp[v] = (int32_t)v;
    best[v] = MST_NONE;
    done[v] = 0;
  }
}

/// done[v]: 0 = walk the row, 1 = every entry is internal, 2 = a big row nobody has found an
/// outgoing entry in (the big kernel writes 0 back when it finds one).  `use_flags` == 0: done[] is
/// neither read nor written and every row is walked in every round.
__global__ void __launch_bounds__(MST_BLOCK)
    mst_search_kernel(const int32_t* ap, const int32_t* aj, const float* ax, const int32_t* comp,
                      unsigned long long* best, unsigned char* done, int32_t n, int use_flags, int32_t big_row,
                      int2* big, mst_counters_t* ctr) {
  __shared__ int32_t s_pre[MST_BLOCK], s_base[MST_BLOCK], s_comp[MST_BLOCK], s_wave[MST_BLOCK / wave_size + 1];
  __shared__ int32_t s_live[MST_BLOCK];
  __shared__ unsigned long long s_sum[MST_BLOCK / wave_size];
  const int tid = threadIdx.x;
  unsigned long long read = 0;
  for (int64_t a = blockIdx.x * (int64_t)MST_BLOCK; a < n; a += (int64_t)gridDim.x * MST_BLOCK) {
    const int64_t v = a + tid;
    int32_t lo = 0, d = 0, c = 0;
    bool walked = false;
    if (v < n && !(use_flags && done[v])) {
      lo = ap[v];
      d = max(ap[v + 1] - lo, 0);
      c = comp[v];
      if (d > big_row) {
        push_big_segments<MST_BIG_SEGMENT>(&ctr->big_n, big, (int32_t)v, d);
        if (use_flags)
          done[v] = 2;
        read += (unsigned long long)d;
        d = 0;
      } else {
        walked = true;
      }
    }
    s_live[tid] = 0;
    s_comp[tid] = c;
    const int32_t P = flat_walk<MST_BLOCK>(d, lo, s_pre, s_base, s_wave, [&](int o, int32_t e) {
      const int32_t cu = s_comp[o], cv = comp[aj[e]];
      if (cu != cv) {
        const unsigned long long key = mst_key(ax[e], e);
        mst_min(best + cu, key);
        mst_min(best + cv, key);
        s_live[o] = 1;
      }
    });
    read += (unsigned long long)(tid == 0 ? P : 0);
    // s_live is complete behind flat_walk's trailing barrier (P == 0: nobody wrote it)
    if (use_flags && walked && !s_live[tid])
      done[v] = 1;
  }
  read = block_sum<MST_BLOCK>(read, s_sum);
  if (tid == 0 && read)
    atomicAdd(&ctr->edges, read);
}

/// The segments on the big list, one workgroup each, consecutive threads on consecutive entries.
/// The row's own component is the same for the whole segment: its keys are reduced per wave first.
__global__ void __launch_bounds__(MST_BLOCK)
    mst_big_kernel(const int32_t* ap, const int32_t* aj, const float* ax, const int32_t* comp,
                   unsigned long long* best, unsigned char* done, int use_flags, const int2* big,
                   const mst_counters_t* ctr) {
  const int32_t items = ctr->big_n;  // written by the search kernel before this one; constant here
  for (int32_t i = blockIdx.x; i < items; i += gridDim.x) {
    const int2 item = big[i];  // {vertex, segment of its row}
    const int32_t u = item.x, cu = comp[u];
    const int64_t lo = (int64_t)ap[u] + (int64_t)item.y * MST_BIG_SEGMENT;
    const int64_t hi = min((int64_t)ap[u + 1], lo + MST_BIG_SEGMENT);
    unsigned long long mine = MST_NONE;
    for (int64_t e = lo + threadIdx.x; e < hi; e += MST_BLOCK) {
      const int32_t cv = comp[aj[e]];
      if (cu != cv) {
        const unsigned long long key = mst_key(ax[e], (int32_t)e);
        mst_min(best + cv, key);
        mine = key < mine ? key : mine;
      }
    }
    mine = wave_min(mine);
    if (lane_id() == 0 && mine != MST_NONE) {
      mst_min(best + cu, mine);
      if (use_flags)
        done[u] = 0;
    }
  }
}

__global__ void __launch_bounds__(MST_BLOCK)
    mst_hook_kernel(const int32_t* ap, const int32_t* aj, const int32_t* comp, const unsigned long long* best,
                    int32_t* link, unsigned int* chosen, int32_t n, mst_counters_t* ctr) {
  __shared__ unsigned long long s_sum[MST_BLOCK / wave_size];
  unsigned long long hooked = 0;
  for (int64_t i = blockIdx.x * (int64_t)MST_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MST_BLOCK) {
    const int32_t r = (int32_t)i;
    if (comp[r] != r)
      continue;
    const unsigned long long key = best[r];
    int32_t to = r;
    if (key != MST_NONE) {
      const int32_t e = (int32_t)(uint32_t)key;
      const int32_t cu = comp[mst_row_of(ap, n, e)], cv = comp[aj[e]];
      const int32_t other = cu == r ? cv : cu;
      // both picked this entry: the smaller root id stays root, the other one records the entry
      if (!(best[other] == key && r < other)) {
        to = other;
        atomicOr(chosen + ((uint32_t)e >> 5), 1u << (e & 31));
        ++hooked;
      }
    }
    link[r] = to;
  }
  hooked = block_sum<MST_BLOCK>(hooked, s_sum);
  if (threadIdx.x == 0 && hooked)
    atomicAdd(&ctr->hooked, hooked);
}

/// Pass `pass` of the round's pointer jumping over the roots the hook kernel wrote.  A word always
/// names an ancestor, a pass at least halves every root's distance to the top, in place or not.
__global__ void __launch_bounds__(MST_BLOCK)
    mst_jump_kernel(const int32_t* comp, int32_t* link, int32_t n, int pass, mst_counters_t* ctr) {
  if (pass > 0 && ctr->changed[pass - 1] == 0)  // written by the kernel before this one
    return;
  bool changed = false;
  for (int64_t v = blockIdx.x * (int64_t)MST_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * MST_BLOCK) {
    if (comp[v] != (int32_t)v)
      continue;
    int32_t l = load_relaxed(link + v), ll = load_relaxed(link + l);
    if (l == ll)
      continue;
    for (int k = 0; k < 4 && l != ll; ++k) {
      l = ll;
      ll = load_relaxed(link + l);
    }
    store_relaxed(link + v, l);
    changed = true;
  }
  if (changed)
    ctr->changed[pass] = 1;  // every writer writes the same value
}

__global__ void __launch_bounds__(MST_BLOCK)
    mst_flatten_kernel(int32_t* comp, const int32_t* link, unsigned long long* best, int32_t n) {
  for (int64_t v = blockIdx.x * (int64_t)MST_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * MST_BLOCK) {
    comp[v] = link[comp[v]];  // comp[v] was a root of this round: the hook kernel wrote its word
    best[v] = MST_NONE;
  }
}

/// Copy the counters to the host's mirror, clear the round's, stamp the hand-off.
__global__ void mst_publish_kernel(mst_counters_t* ctr, unsigned long long* mirror, int sequence_slot,
                                   unsigned long long sequence) {
  if (threadIdx.x == 0) {
    mirror[MST_EDGES] = ctr->edges;
    mirror[MST_HOOKED] = ctr->hooked;
    mirror[MST_COUNT] = ctr->count;
    mirror[MST_WEIGHT] = (unsigned long long)__double_as_longlong(ctr->weight);
    ctr->hooked = 0;
    ctr->big_n = 0;
    for (int j = 0; j < MST_MAX_JUMPS; ++j)
      ctr->changed[j] = 0;
    stamp_handoff(mirror, sequence_slot, sequence);
  }
}

// ---- labels: the smallest vertex id of each component (what grx_cc returns) ----------------------

__global__ void __launch_bounds__(MST_BLOCK) mst_minid_init_kernel(int32_t* smallest, int32_t n) {
  for (int64_t v = blockIdx.x * (int64_t)MST_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * MST_BLOCK)
    smallest[v] = (int32_t)v;
}

__global__ void __launch_bounds__(MST_BLOCK) mst_minid_kernel(const int32_t* comp, int32_t* smallest, int32_t n) {
  for (int64_t v = blockIdx.x * (int64_t)MST_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * MST_BLOCK) {
    const int32_t c = comp[v];
    if ((int32_t)v < c && load_relaxed(smallest + c) > (int32_t)v)
      atomicMin(smallest + c, (int32_t)v);
  }
}

__global__ void __launch_bounds__(MST_BLOCK)
    mst_label_kernel(const int32_t* comp, const int32_t* smallest, int32_t* label, int32_t n) {
  for (int64_t v = blockIdx.x * (int64_t)MST_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * MST_BLOCK)
    label[v] = smallest[comp[v]];
}

// ---- the bitmap to ascending positions, and the weights' sum --------------------------------------
// A tile is MST_BLOCK words of the bitmap (a word per thread); whichever workgroup takes a tile
// computes the same numbers, so nothing below depends on the schedule.

__global__ void __launch_bounds__(MST_BLOCK)
    mst_tile_count_kernel(const unsigned int* chosen, int64_t words, int64_t tiles, unsigned int* tile_count) {
  __shared__ unsigned long long s_sum[MST_BLOCK / wave_size];
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t w = t * MST_BLOCK + threadIdx.x;
    const unsigned long long c = block_sum<MST_BLOCK>(w < words ? (unsigned long long)__popc(chosen[w]) : 0ull, s_sum);
    if (threadIdx.x == 0)
      tile_count[t] = (unsigned int)c;
    __syncthreads();  // the next tile rewrites s_sum
  }
}

/// ONE workgroup: tile_count[] becomes its exclusive prefix, the total goes to the counters.
__global__ void __launch_bounds__(MST_SCAN_BLOCK)
    mst_tile_scan_kernel(unsigned int* tile_count, int64_t tiles, mst_counters_t* ctr) {
  __shared__ unsigned long long s_wave[MST_SCAN_BLOCK / wave_size + 1];
  unsigned long long carry = 0;
  for (int64_t base = 0; base < tiles; base += MST_SCAN_BLOCK) {
    const int64_t t = base + threadIdx.x;
    const unsigned long long x = t < tiles ? tile_count[t] : 0;
    unsigned long long total = 0;
    const unsigned long long excl = block_exclusive_sum<MST_SCAN_BLOCK>(x, total, s_wave);
    if (t < tiles)
      tile_count[t] = (unsigned int)(carry + excl);
    carry += total;
  }
  if (threadIdx.x == 0)
    ctr->count = carry;
}

/// Sum of one double per thread in a fixed tree, valid in thread 0.  `s`: BLOCK doubles of LDS.
template <int BLOCK>
__device__ __forceinline__ double mst_tree_sum(double x, double* s) {
  s[threadIdx.x] = x;
  __syncthreads();
  for (int half = BLOCK / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half)
      s[threadIdx.x] += s[threadIdx.x + half];
    __syncthreads();
  }
  return s[0];
}

/// entries (may be NULL): position `tile_offset[tile] + rank` gets the rank-th chosen entry of the
/// tile, so the whole array ascends.  tile_sum[tile]: the float64 sum of the tile's chosen weights,
/// each thread's in ascending position, the threads' in a fixed tree.
__global__ void __launch_bounds__(MST_BLOCK)
    mst_emit_kernel(const unsigned int* chosen, const float* ax, int64_t words, int64_t tiles,
                    const unsigned int* tile_offset, int32_t* entries, int64_t capacity, double* tile_sum) {
  __shared__ unsigned int s_wave[MST_BLOCK / wave_size + 1];
  __shared__ double s_tree[MST_BLOCK];
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t w = t * MST_BLOCK + threadIdx.x;
    unsigned int bits = w < words ? chosen[w] : 0u;
    unsigned int total = 0;
    int64_t at = (int64_t)tile_offset[t] + block_exclusive_sum<MST_BLOCK>((unsigned int)__popc(bits), total, s_wave);
    double sum = 0.0;
    while (bits) {
      const int b = __ffs(bits) - 1;
      bits &= bits - 1;
      const int64_t e = w * 32 + b;
      if (entries && at < capacity)
        entries[at] = (int32_t)e;
      ++at;
      sum += (double)ax[e];
    }
    sum = mst_tree_sum<MST_BLOCK>(sum, s_tree);
    if (threadIdx.x == 0)
      tile_sum[t] = sum;
    __syncthreads();  // the next tile rewrites s_tree
  }
}

/// ONE workgroup: thread i adds tiles i, i + BLOCK, ... in that order, then the fixed tree.
__global__ void __launch_bounds__(MST_SCAN_BLOCK)
    mst_sum_kernel(const double* tile_sum, int64_t tiles, mst_counters_t* ctr) {
  __shared__ double s_tree[MST_SCAN_BLOCK];
  double sum = 0.0;
  for (int64_t t = threadIdx.x; t < tiles; t += MST_SCAN_BLOCK)
    sum += tile_sum[t];
  sum = mst_tree_sum<MST_SCAN_BLOCK>(sum, s_tree);
  if (threadIdx.x == 0)
    ctr->weight = sum;
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

/**
 * @file cc_kernels.hxx
 * @brief Connected components (grx_cc): Afforest (Sutton, Ben-Nun, Barak 2018) -- lock-free
 * union-find on parent[V], neighbour sampling, and a remainder pass that leaves the rows of the
 * largest component unread.
 *
 * State: parent[V], kept in the caller's output array.  Invariant: parent[v] <= v.  It holds after
 * cc_init_kernel (parent[v] = v), a hook writes the SMALLER root into the larger one's word, and a
 * compress step replaces a parent by an ancestor.  So every tree's root is its smallest member, and
 * the fully compressed array is the answer: the smallest vertex id of each component, whoever won
 * which race.
 *
 *   cc_init_kernel       parent[v] = v.
 *   cc_sample_kernel     neighbour round r: every vertex with more than r entries hooks to entry r
 *                        of its row.  One thread per vertex.
 *   cc_compress_kernel   parent[v] = root of v (no hook runs beside it, so roots stand still);
 *                        COUNT: the roots are counted as well (the last pass of a call).
 *   cc_pick_kernel       ONE workgroup reads parent at CC_SAMPLES evenly spread positions and
 *                        leaves the most frequent value (ties: the smaller) in the counters.
 *   cc_remainder_kernel  a chunk of CC_BLOCK consecutive vertices per workgroup: the entries from
 *                        position `first` on of every vertex whose parent is not the picked one,
 *                        flattened over the workgroup's threads (flat_walk, row_walk.hxx).
 *                        Rows with more than `big_row` entries left go to a list, cut into
 *                        segments of CC_BIG_SEGMENT entries ...
 *   cc_big_kernel        ... which the grid walks a workgroup per segment, 16 bytes of the row per
 *                        thread: no launch is as long as its longest row.
 *   cc_publish_kernel    copies the counters to the host's mirror and stamps the hand-off.
 *
 * Every read of parent[] inside cc_link and the compress loop is a relaxed agent-scope atomic load: other
 * CUs change these words while the kernel runs, and a plain load may be answered by the CU's L1 for
 * ever, or be hoisted out of the loop.  A stale value costs another trip; the compare-and-swap
 * decides.
 */
#pragma once

#include <gunrock/hip/kernels/row_walk.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int CC_BLOCK = 256;
constexpr int CC_SAMPLES = 1024;       // positions the pick reads; also its workgroup size
constexpr int CC_SAMPLE_ROUNDS = 2;    // default neighbour rounds
constexpr int CC_MAX_ROUNDS = 8;
constexpr int CC_BIG_ROW = 4096;       // default: rows with more entries left go to the big list ...
constexpr int CC_BIG_SEGMENT = 4096;   // ... in segments of this many entries, a workgroup each
constexpr int32_t CC_NO_GIANT = -1;    // no vertex has this parent: every row is walked

/// Device counters of one grx_cc call.
struct cc_counters_t {
  unsigned long long edges;       // row entries the hooking kernels read
  unsigned long long components;  // roots after the last compress
  int giant;                      // the picked parent (cc_pick_kernel)
  int big_n;                      // segments on the big list
};
/// What the host reads at the hand-off (words of the pinned mirror).
enum { CC_EDGES = 0, CC_COMPONENTS, CC_GIANT, CC_WORDS };

/// Join the trees of u and v: the larger root is hooked under the smaller.  Every trip moves up a
/// tree or ends, and trees are finite (parent[x] < x below a root).
__device__ __forceinline__ void cc_link(int32_t* parent, int32_t u, int32_t v) {
  int32_t p1 = load_relaxed(parent + u), p2 = load_relaxed(parent + v);
  while (p1 != p2) {
    const int32_t high = p1 > p2 ? p1 : p2, low = p1 > p2 ? p2 : p1;
    const int32_t p_high = load_relaxed(parent + high);
    if (p_high == low)
      break;
    if (p_high == high && atomicCAS(parent + high, high, low) == high)
      break;
    p1 = load_relaxed(parent + load_relaxed(parent + high));
    p2 = load_relaxed(parent + low);
  }
}

__global__ void __launch_bounds__(CC_BLOCK) cc_init_kernel(int32_t* parent, int32_t n) {
  for (int64_t v = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * CC_BLOCK)
    parent[v] = (int32_t)v;
}

__global__ void __launch_bounds__(CC_BLOCK)
    cc_sample_kernel(const int32_t* ap, const int32_t* aj, int32_t* parent, int32_t n, int32_t r, cc_counters_t* ctr) {
  __shared__ unsigned long long s_wave[CC_BLOCK / wave_size];
  unsigned long long read = 0;
  for (int64_t v = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * CC_BLOCK) {
    const int32_t lo = ap[v];
    if (ap[v + 1] - lo > r) {
      cc_link(parent, (int32_t)v, aj[lo + r]);
      ++read;
    }
  }
  read = block_sum<CC_BLOCK>(read, s_wave);
  if (threadIdx.x == 0 && read)
    atomicAdd(&ctr->edges, read);
}

template <bool COUNT>
__global__ void __launch_bounds__(CC_BLOCK) cc_compress_kernel(int32_t* parent, int32_t n, cc_counters_t* ctr) {
  __shared__ unsigned long long s_wave[CC_BLOCK / wave_size];
  unsigned long long roots = 0;
  const int lane = lane_id();
  const int64_t stride = (int64_t)gridDim.x * CC_BLOCK;
  // whole wavefronts run every trip: the ballot below sees all 64 lanes
  for (int64_t v0 = blockIdx.x * (int64_t)CC_BLOCK + threadIdx.x - lane; v0 < n; v0 += stride) {
    const int64_t v = v0 + lane;
    bool root = false;
    if (v < n) {
      // a racing compress writes an ancestor either way; the chain above p only gets shorter
      int32_t p = load_relaxed(parent + v), pp = load_relaxed(parent + p);
      const int32_t was = p;
      while (p != pp) {
        p = pp;
        pp = load_relaxed(parent + p);
      }
      if (p != was)
        store_relaxed(parent + v, p);
      root = p == (int32_t)v;
    }
    if (COUNT) {
      const unsigned long long m = __ballot(root);
      if (lane == 0)
        roots += (unsigned long long)__popcll(m);
    }
  }
  if (COUNT) {
    roots = block_sum<CC_BLOCK>(roots, s_wave);
    if (threadIdx.x == 0 && roots)
      atomicAdd(&ctr->components, roots);
  }
}

/// The most frequent parent among CC_SAMPLES fixed positions (no random numbers: the answer does not
/// depend on the pick, only the work does).  Runs after a compress: the values are roots.
__global__ void __launch_bounds__(CC_SAMPLES) cc_pick_kernel(const int32_t* parent, int32_t n, cc_counters_t* ctr) {
  __shared__ int32_t s_value[CC_SAMPLES];
  __shared__ unsigned long long s_best;
  const int tid = threadIdx.x;
  const int32_t mine = parent[(int64_t)tid * n / CC_SAMPLES];
  s_value[tid] = mine;
  if (tid == 0)
    s_best = 0;
  __syncthreads();
  unsigned count = 0;
  for (int i = 0; i < CC_SAMPLES; ++i)  // every lane reads the same word: a broadcast
    count += s_value[i] == mine;
  // the larger count wins, then the smaller value
  const unsigned long long key = ((unsigned long long)count << 32) | (0x7fffffffu - (unsigned)mine);
  atomicMax(&s_best, key);
  __syncthreads();
  if (tid == 0)
    ctr->giant = (int32_t)(0x7fffffffu - (unsigned)(s_best & 0xffffffffu));
}

/// `use_giant`: the picked parent is read from the counters (the pick ran in this batch of launches);
/// otherwise no row is left out.
__global__ void __launch_bounds__(CC_BLOCK)
    cc_remainder_kernel(const int32_t* ap, const int32_t* aj, int32_t* parent, int32_t n, int32_t first, int use_giant,
                        int32_t big_row, int2* big, cc_counters_t* ctr) {
  __shared__ int32_t s_pre[CC_BLOCK], s_base[CC_BLOCK], s_wave[CC_BLOCK / wave_size + 1];
  __shared__ unsigned long long s_sum[CC_BLOCK / wave_size];
  const int tid = threadIdx.x;
  const int32_t giant = use_giant ? ctr->giant : CC_NO_GIANT;  // written by an earlier kernel
  unsigned long long read = 0;
  for (int64_t a = blockIdx.x * (int64_t)CC_BLOCK; a < n; a += (int64_t)gridDim.x * CC_BLOCK) {
    const int64_t v = a + tid;
    int32_t lo = 0, d = 0;
    if (v < n && load_relaxed(parent + v) != giant) {
      lo = ap[v] + first;
      d = max(ap[v + 1] - lo, 0);
      if (d > big_row) {
        push_big_segments<CC_BIG_SEGMENT>(&ctr->big_n, big, (int32_t)v, d);
        read += (unsigned long long)d;
        d = 0;
      }
    }
    // P == 0: the whole chunk is in the picked component, or has nothing left
    const int32_t P = flat_walk<CC_BLOCK>(d, lo, s_pre, s_base, s_wave,
                                          [&](int o, int32_t e) { cc_link(parent, (int32_t)a + o, aj[e]); });
    read += (unsigned long long)(tid == 0 ? P : 0);
  }
  read = block_sum<CC_BLOCK>(read, s_sum);
  if (tid == 0 && read)
    atomicAdd(&ctr->edges, read);
}

/// The segments on the big list, one workgroup each: the part of a segment between 16-byte
/// boundaries four entries per thread, its ends one entry per thread.
__global__ void __launch_bounds__(CC_BLOCK)
    cc_big_kernel(const int32_t* ap, const int32_t* aj, int32_t* parent, int32_t first, const int2* big,
                  const cc_counters_t* ctr) {
  const int32_t items = ctr->big_n;  // written by the remainder kernel before this one; constant here
  const int64_t me = threadIdx.x;
  for (int32_t i = blockIdx.x; i < items; i += gridDim.x) {
    const int2 item = big[i];  // {vertex, segment of its row}
    const int32_t u = item.x;
    const int64_t row_hi = ap[u + 1];
    const int64_t lo = (int64_t)ap[u] + first + (int64_t)item.y * CC_BIG_SEGMENT;
    const int64_t hi = min(row_hi, lo + CC_BIG_SEGMENT);
    // [lo, head) and [tail, hi) are the ends, [head, tail) is whole 16-byte words
    const int64_t skew = (int64_t)((reinterpret_cast<uintptr_t>(aj + lo) >> 2) & 3);
    const int64_t head = min(hi, lo + ((4 - skew) & 3));
    const int64_t tail = head + ((hi - head) & ~(int64_t)3);
    for (int64_t q = me; q < (tail - head) / 4; q += CC_BLOCK) {
      const int4 w = *reinterpret_cast<const int4*>(aj + head + 4 * q);
      cc_link(parent, u, w.x);
      cc_link(parent, u, w.y);
      cc_link(parent, u, w.z);
      cc_link(parent, u, w.w);
    }
    const int64_t ends = (head - lo) + (hi - tail);  // at most 6
    if (me < ends)
      cc_link(parent, u, aj[me < head - lo ? lo + me : tail + (me - (head - lo))]);
  }
}

/// Copy the counters to the host's mirror and stamp the hand-off: the last kernel of a call.
__global__ void cc_publish_kernel(const cc_counters_t* ctr, unsigned long long* mirror, int sequence_slot,
                                  unsigned long long sequence) {
  if (threadIdx.x == 0) {
    mirror[CC_EDGES] = ctr->edges;
    mirror[CC_COMPONENTS] = ctr->components;
    mirror[CC_GIANT] = (unsigned long long)(long long)ctr->giant;
    stamp_handoff(mirror, sequence_slot, sequence);
  }
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

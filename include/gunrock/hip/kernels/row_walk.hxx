/**
 * @file row_walk.hxx
 * @brief What the kernels of the non-traversal algorithms (cc, mst, kcore, color) share: the stamp
 * that ends a publish kernel, the split of a long row into segments for whole workgroups, and the
 * walk over a chunk's rows flattened across the workgroup's threads.
 *
 * flat_walk runs its body for entries only and leaves early when the chunk has none.  A body that
 * appends to a queue holds a ballot and needs whole wavefronts: that walk is queue_walk
 * (generation_queue.hxx), whose big list holds whole rows.
 */
#pragma once

#include <gunrock/hip/primitives.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

/// Stamp the hand-off: ONE thread, after it has written its words of the host's mirror.
__device__ __forceinline__ void stamp_handoff(unsigned long long* mirror, int sequence_slot,
                                              unsigned long long sequence) {
  __threadfence_system();
  __hip_atomic_store(&mirror[sequence_slot], sequence, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

/// The 32-bit finaliser: a bijection on the unsigned vertex id (the tie-break of color's and scc's keys).
__host__ __device__ __forceinline__ unsigned fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

/// Put the d entries of row v on the big list as ceil(d / SEGMENT) items {v, segment}.
template <int SEGMENT>
__device__ __forceinline__ void push_big_segments(int* big_n, int2* big, int32_t v, int32_t d) {
  const int32_t segments = (d + SEGMENT - 1) / SEGMENT;
  const int32_t at = atomicAdd(big_n, segments);
  for (int32_t k = 0; k < segments; ++k)
    big[at + k] = make_int2(v, k);
}

/**
 * @brief The rows of a chunk of BLOCK owners flattened over the workgroup: thread `tid` brings the d
 * entries from position lo on of owner `tid`; body(owner, position) runs once per entry, consecutive
 * threads on consecutive entries.  Returns the chunk's entries P.  Every thread of the workgroup
 * calls it.  When P == 0 no LDS is touched and there is no barrier beyond the prefix sum's two;
 * otherwise what the caller wrote to LDS before the call is visible to body, and a trailing barrier
 * lets the next chunk rewrite the prefix.  `s_pre`, `s_base`: BLOCK words; `s_wave`: BLOCK / 64 + 1.
 */
template <int BLOCK, typename body_t>
__device__ __forceinline__ int32_t flat_walk(int32_t d, int32_t lo, int32_t* s_pre, int32_t* s_base, int32_t* s_wave,
                                             body_t&& body) {
  const int tid = threadIdx.x;
  int32_t P = 0;
  const int32_t excl = block_exclusive_sum<BLOCK>(d, P, s_wave);
  if (P == 0)  // uniform
    return 0;
  s_pre[tid] = excl + d;
  s_base[tid] = lo - excl;
  __syncthreads();
  for (int32_t t = tid; t < P; t += BLOCK) {
    const int o = prefix_owner(s_pre, BLOCK, t);
    body(o, s_base[o] + t);
  }
  __syncthreads();
  return P;
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

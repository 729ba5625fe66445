/**
 * @file hand_off.hxx
 * @brief How every operator and batch call hands the context's device counters to the host, sizes a
 * grid and times its kernels.  Used by advance, filter, the partitioned supersteps and the C ABI.
 */
#pragma once

#include <gunrock/hip/context.hxx>

#include <atomic>

namespace gunrock {
namespace hip {

inline unsigned grid_for(std::size_t items, std::size_t per_block, unsigned cap = 0x7fffffffu) {
  std::size_t g = (items + per_block - 1) / per_block;
  if (g < 1)
    g = 1;
  return (unsigned)(g > cap ? cap : g);
}

/**
 * @brief Hand the device counters to the host WITHOUT a memcpy command, a memset command or a
 * stream-synchronise call: a one-lane kernel copies the first 16 counters into the pinned
 * mirror, zeroes them for the next operator and then stores a sequence number; the host spins
 * on that word.  (The reference pays a thrust reduce + D2H + cudaStreamSynchronize + a
 * cudaMalloc'ed cursor per advance: block_mapped.hxx:160-204.)  Invariant: counters 0..15 are
 * zero whenever no operator is in flight.
 */
template <int header_only = 0>  // a template so that every translation unit may define it
__global__ void publish_counters_kernel(unsigned long long* counters, unsigned long long* mirror,
                                        unsigned long long sequence, long long* copy_to,
                                        int copy_slot, unsigned long long* zero_this) {
  const int i = threadIdx.x;
#ifdef GRX_TILE_TIMING
  if (i < 31) {  // diagnostic build: slots 24..30 carry the tile kernel's phase clocks
#else
  if (i < 24) {  // 0..15 operator counters, 16..23 tile-pool cursors
#endif
    // the counters were updated by device-scope atomics (memory side); read and clear them
    // with cache-bypassing accesses instead of trusting what this XCD's L2 may still hold
    const unsigned long long value =
        __hip_atomic_exchange(&counters[i], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    mirror[i] = value;
    // fused pipelines: leave one counter where the next device-side consumer reads it (a send
    // slot's header) and clear one device word (a frontier length the next admit accumulates)
    if (copy_to && i == copy_slot)
      *copy_to = (long long)value;
  }
  if (zero_this && i == 32)
    __hip_atomic_store(zero_this, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence_system();
  __syncthreads();
  if (i == 0) {
    __hip_atomic_store(&mirror[gcuda::workspace_t::sequence_slot], sequence, __ATOMIC_RELEASE,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

/// Enqueue the hand-off (copy to the mirror, clear, stamp); returns the sequence number.
inline unsigned long long publish_counters(gcuda::standard_context_t& ctx, long long* copy_to = nullptr,
                                           int copy_slot = 0,
                                           unsigned long long* zero_this = nullptr) {
  auto& ws = ctx.workspace();
  const unsigned long long seq = ws.next_sequence();
  publish_counters_kernel<0><<<1, 64, 0, ctx.stream()>>>(ws.counters(), ws.mirror(), seq, copy_to,
                                                         copy_slot, zero_this);
  GRX_HIP_CHECK(hipGetLastError());
  return seq;
}

/// Wait until hand-off `seq` has landed; returns the pinned mirror.
inline unsigned long long* await_counters(gcuda::standard_context_t& ctx, unsigned long long seq) {
  auto& ws = ctx.workspace();
  volatile unsigned long long* flag = ws.mirror() + gcuda::workspace_t::sequence_slot;
  unsigned spins = 0;
  while (*flag < seq) {
    __builtin_ia32_pause();
    if ((++spins & 0xFFFFu) == 0) {
      // every ~100 us: make sure the stream is still healthy (a faulted kernel never publishes)
      hipError_t st = hipStreamQuery(ctx.stream());
      if (st != hipSuccess && st != hipErrorNotReady)
        error::throw_if_exception(st, "operator kernels failed");
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return ws.mirror();
}

/// Publish the counters and wait for them; returns the pinned mirror.
inline unsigned long long* fetch_counters(gcuda::standard_context_t& ctx) {
  return await_counters(ctx, publish_counters(ctx));
}

struct clocked_t {
  gcuda::standard_context_t& ctx;
  explicit clocked_t(gcuda::standard_context_t& c) : ctx(c) {
    if (ctx.options().time_kernels)
      ctx.kernel_clock().start(ctx.stream());
  }
  void stop() {
    if (ctx.options().time_kernels)
      ctx.kernel_clock().stop(ctx.stream());
  }
};

}  // namespace hip
}  // namespace gunrock

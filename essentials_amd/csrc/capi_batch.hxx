/**
 * @file capi_batch.hxx
 * @brief Host scaffold of the calls that are batches of their own kernels rather than operator
 * pipelines (grx_tc, grx_kcore, grx_cc, grx_mst; grx_bc takes the grid and the clock): test hooks,
 * grid sizing, the call's clock, the hand-off that ends a batch, the symmetric-CSR gate.  Not installed.
 */
#pragma once

#include "capi_internal.hxx"

#include <cstdlib>

namespace essentials_amd {

/// A test hook: the integer in environment variable `name` clamped to [lo, hi]; `fallback` when unset.
inline long long env_or(const char* name, long long fallback, long long lo, long long hi) {
  if (const char* e = std::getenv(name))
    return std::max(lo, std::min(hi, std::atoll(e)));
  return fallback;
}

/// Workgroups for `items` at `per_block` each: at least one, at most eight per CU.
inline unsigned grid_for(std::size_t items, std::size_t per_block, gcuda::standard_context_t& ctx) {
  return operators::advance::detail::grid_for(items, per_block, (unsigned)ctx.compute_units() * 8u);
}

/// The two clocks of a call: the whole call (grx_stats::elapsed_ms) and, when `timed`
/// (collect_kernel_time), the sum over its batches of launches (advance_kernel_ms).  The batch
/// events are created on first use and re-recorded per batch: an interval is collected when the
/// next one begins or the sum is read, both behind a host wait for the batch's last kernel.
class call_clock_t {
 public:
  call_clock_t(hipStream_t stream, bool timed) : call_(stream), stream_(stream), timed_(timed) {}
  void start() { call_.begin(); }
  void stop_and_wait() { call_.end(); }
  float elapsed_ms() const { return call_.milliseconds(); }
  void begin_batch() {
    if (timed_) {
      batches_.collect();
      batches_.start(stream_);
    }
  }
  void end_batch() {
    if (timed_)
      batches_.stop(stream_);
  }
  float kernel_ms() {
    batches_.collect();
    return batches_.total_ms;
  }

 private:
  util::timer_t call_;
  gcuda::kernel_clock_t batches_;
  hipStream_t stream_;
  bool timed_;
};

/// End a batch of launches: `publish(mirror, sequence_slot, sequence)` launches the kernel that
/// copies the call's counters to the mirror and stamps it; returns the mirror once the stamp landed.
template <typename publish_t>
unsigned long long* hand_off(gcuda::standard_context_t& sc, call_clock_t& clock, publish_t&& publish) {
  auto& ws = sc.workspace();
  const unsigned long long seq = ws.next_sequence();
  publish(ws.mirror(), (int)gcuda::workspace_t::sequence_slot, seq);
  GRX_HIP_CHECK(hipGetLastError());
  clock.end_batch();
  return operators::advance::detail::await_counters(sc, seq);
}

/// Undirected input only: an attached transpose marks the graph directed, and a graph nobody has
/// vouched for is verified once (ensure_can_pull returns OK when in-edges are attached).  GRX_OK or
/// GRX_ERR_UNSUPPORTED with the message set.  Call inside guarded().
inline int require_symmetric(grx_context_s* ctx, grx_graph_s* g, const char* call, const char* what) {
  const char* found = nullptr;
  if (g->in_edges)
    found = "the graph has in-edges attached";
  else if (ensure_can_pull(ctx, g) != GRX_OK)
    found = "the CSR is not symmetric";
  if (!found)
    return GRX_OK;
  return unsupported((std::string(call) + ": " + found + " (directed); " + what + " needs a symmetric CSR").c_str());
}

}  // namespace essentials_amd

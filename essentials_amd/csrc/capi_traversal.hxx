/**
 * @file capi_traversal.hxx
 * @brief What the calls that run an enactor of clients.hxx share (grx_bfs, grx_sssp, grx_pagerank,
 * grx_bc's search): the graph a call runs on, the run of the BFS client, and the stats of a run.
 * Not installed.
 */
#pragma once

#include "capi_internal.hxx"
#include "clients.hxx"

namespace essentials_amd {

/// The graph a call runs on: the caller's, or its hot-first renumbered copy (reorder.hxx) with what
/// translates between the two numberings (null on the caller's own graph).
struct run_graph_t {
  grx_graph_s* on;
  const int32_t* scatter_to;   ///< device: the caller's id of a renumbered vertex
  const int32_t* gather_from;  ///< device: the renumbered id of a caller's vertex
  const int32_t* rank_of;      ///< host: the same
  bool renumbered() const { return rank_of != nullptr; }
  int32_t vertex(int32_t callers) const { return rank_of ? rank_of[(std::size_t)callers] : callers; }
};

/// `may_copy`: the call's own condition for running on the copy; hot_copy() has the last word
/// (`csr_only`: see there).  Call inside guarded().
inline run_graph_t run_graph(grx_context_s* ctx, grx_graph_s* g, bool may_copy, bool csr_only = false) {
  if (may_copy)
    if (grx_graph_s* h = hot_copy(ctx, g, csr_only))
      return {h, g->hot_vertex_of.data(), g->hot_rank_of_device.data(), g->hot_rank_of.data()};
  return {g, nullptr, nullptr, nullptr};
}

/// One run of the BFS client on a freshly constructed `problem`: the direction-optimising enactor
/// or the push enactor, as the options say.
struct bfs_run_t {
  float ms = 0;
  int iterations = 0, pulls = 0;
};
template <operators::load_balance_t lb, typename problem_t>
bfs_run_t run_bfs_client(problem_t& problem, int64_t n_rows, const grx_options& o, grx_context_s* ctx) {
  // push search: one byte per vertex while it runs once 4-byte depths outgrow the eight L2s
  // (GRX_BFS_BYTE_LABELS=0/1 overrides; measurements in DESIGN.md, "Larger graphs")
  if (!o.direction_optimized)
    problem.byte_labels = env_flag("GRX_BFS_BYTE_LABELS", n_rows > (1ll << 22));
  problem.init();
  problem.reset();
  enactor_properties_t props;
  if (o.frontier_sizing_factor > 0)
    props.frontier_sizing_factor = o.frontier_sizing_factor;
  bfs_run_t run;
  if (o.direction_optimized) {
    clients::bfs_do_enactor_t<problem_t, lb> enactor(&problem, ctx->mc, props);
    enactor.max_iterations = o.max_iterations;
    if (o.do_alpha > 0) enactor.alpha = o.do_alpha;
    if (o.do_beta > 0) enactor.beta = o.do_beta;
    run.ms = enactor.enact();
    run.iterations = enactor.iteration;
    run.pulls = enactor.pull_iterations;
  } else {
    clients::bfs_enactor_t<problem_t, lb> enactor(&problem, ctx->mc, props);
    enactor.max_iterations = o.max_iterations;
    enactor.mark_without_claim = env_flag("GRX_BFS_MARK", enactor.mark_without_claim);
    // wide levels of a graph KNOWN to be symmetric pull (no symmetry check is run for this)
    enactor.pull_wide_levels = env_flag("GRX_BFS_PULL", enactor.pull_wide_levels);
    if (o.do_alpha > 0) enactor.alpha = o.do_alpha;
    run.ms = enactor.enact();
    run.iterations = enactor.iteration;
    run.pulls = enactor.pull_iterations;
  }
  return run;
}

/// The stats every enactor run reports (the rest zero): its time, its iterations, the kernel clock.
inline void run_stats(grx_stats* stats, float ms, int iterations, gcuda::standard_context_t& sc) {
  std::memset(stats, 0, sizeof *stats);
  stats->elapsed_ms = ms;
  stats->iterations = iterations;
  stats->advance_kernel_ms = sc.kernel_clock().total_ms;
  stats->advance_launches = sc.kernel_clock().launches;
}
/// ... and the level log of a traversal (clients::level_log_t), as far as grx_stats has room.
inline void level_stats(grx_stats* stats, const clients::level_log_t& log) {
  stats->levels_recorded = log.levels < 64 ? log.levels : 64;
  for (int i = 0; i < stats->levels_recorded; ++i)
    stats->frontier_slots[i] = log.input_slots[i];
}

}  // namespace essentials_amd

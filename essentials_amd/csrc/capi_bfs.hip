/** @file capi_bfs.hip  grx_bfs == gunrock::bfs::run (reference algorithms/bfs.hxx:151-176). */
#include "capi_traversal.hxx"

using namespace essentials_amd;

extern "C" int grx_bfs(grx_context_t ctx, grx_graph_t g, int32_t source, int32_t* d_distances,
                       int32_t* /*d_predecessors*/, const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g || !d_distances)
    return invalid("grx_bfs: NULL argument");
  if (source < 0 || source >= g->n_rows)
    return invalid("grx_bfs: source out of range");
  grx_options o = effective_options(opt);
  return guarded([&] {
    return with_load_balance(o.load_balance, [&](auto lb_tag) -> int {
      constexpr auto lb = decltype(lb_tag)::value;
      using problem_type = clients::bfs_problem_t<graph_type>;
      if (o.direction_optimized)
        if (int rc = ensure_can_pull(ctx, g))
          return rc;
      scoped_options scope(ctx->single(), &o);
      // the search runs on the hot-first renumbered copy of the graph (reorder.hxx) and delivers
      // its depths in the caller's numbering; the form that stands for the unchanged reference
      // client (call_every_edge) and the holes layout keep the caller's graph
      const run_graph_t run = run_graph(ctx, g, !o.call_every_edge && !o.holes_layout);
      graph_type G = run.on->view();
      problem_type problem(G, run.vertex(source), d_distances, ctx->mc);
      problem.scatter_to = run.scatter_to;
      problem.gather_from = run.gather_from;
      const bfs_run_t ran = run_bfs_client<lb>(problem, g->n_rows, o, ctx);
      if (stats) {
        run_stats(stats, ran.ms, ran.iterations, ctx->single());
        stats->pull_iterations = ran.pulls;
        level_stats(stats, problem.log);
        // the first frontier ({source}) carries no work hint: add the source's own degree.  A push
        // search with packed frontiers discovers every vertex exactly once and every level's frontier
        // came with the degree sum of its vertices: the counts are sums over the level log, the
        // source's degree was left in pinned memory by the reset pass -- no statistics pass
        const unsigned long long* facts = ctx->single().workspace().run_facts();
        // (not on a renumbered copy with sinks: a label-scan level labels them without ever putting
        // them into a frontier, so the frontier lengths undercount what was reached)
        if (!o.direction_optimized && !o.holes_layout && o.max_iterations == 0 &&
            problem.log.unknown_work_levels == 1 && !(run.renumbered() && run.on->edges_into_tail)) {
          stats->vertices_reached = problem.log.slots_total;
          stats->edges_traversed = problem.log.edges_expanded + (long long)facts[0];
          stats->edges_expanded = stats->edges_traversed;
        } else {
          stats->edges_expanded = problem.log.edges_expanded +
                                  reach_stats(g, d_distances, (int32_t)INT32_MAX, source, ctx->single(), stats);
        }
      }
      return (int)GRX_OK;
    });
  });
}

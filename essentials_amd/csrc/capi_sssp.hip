/** @file capi_sssp.hip  grx_sssp == gunrock::sssp::run (reference algorithms/sssp.hxx:155-185). */
#include "capi_traversal.hxx"

using namespace essentials_amd;

namespace essentials_amd {
/// Largest |V| for which grx_sssp keeps packed 64-bit labels (GRX_SSSP_PACKED_MAX_VERTICES overrides).
inline long long packed_sssp_max_vertices() {
  // 32 MB of labels: what the eight 4 MB L2s hold between them
  return env_or("GRX_SSSP_PACKED_MAX_VERTICES", 1ll << 22, LLONG_MIN, LLONG_MAX);
}
}  // namespace essentials_amd

extern "C" int grx_sssp(grx_context_t ctx, grx_graph_t g, int32_t source, float* d_distances,
                        int32_t* /*d_predecessors*/, const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g || !d_distances)
    return invalid("grx_sssp: NULL argument");
  if (source < 0 || source >= g->n_rows)
    return invalid("grx_sssp: source out of range");
  grx_options o = effective_options(opt);
  return guarded([&] {
    return with_load_balance(o.load_balance, [&](auto lb_tag) -> int {
      constexpr auto lb = decltype(lb_tag)::value;
      using problem_type = clients::sssp_problem_t<graph_type>;
      using enactor_type = clients::sssp_enactor_t<problem_type, lb>;
      scoped_options scope(ctx->single(), &o);
      // hot-first renumbered copy, distances delivered in the caller's numbering (see grx_bfs); the
      // reference's two-pass formulation and the every-edge form keep the caller's graph
      const run_graph_t run = run_graph(ctx, g, !o.sssp_two_pass && !o.call_every_edge && !o.holes_layout);
      graph_type G = run.on->view();
      problem_type problem(G, run.vertex(source), d_distances, ctx->mc);
      problem.scatter_to = run.scatter_to;
      problem.gather_from = run.gather_from;
      // one 64-bit label per vertex (one RMW per improvement) while 8 bytes per vertex stay
      // cache-sized; beyond that the doubled label footprint costs more lookups that miss than the
      // saved RMWs are worth.  Measured crossover on R-MAT (tools/sssp_packed_vs_words.py, mean
      // enact of 3 sources, packed / two words): scale 20 1.25 / 1.42 ms, 22 2.92 / 3.11, 23 5.56 /
      // 5.46, 24 12.8 / 11.0, 26 58.2 / 53.5.  GRX_SSSP_PACKED=0/1 overrides; the reference's
      // two-pass formulation keeps its two arrays.
      const bool packed = env_flag("GRX_SSSP_PACKED", g->n_rows <= essentials_amd::packed_sssp_max_vertices());
      problem.packed_labels = packed && o.sssp_two_pass == 0;
      // the unpacking pass at the end of a packed run also counts what the run reached
      problem.collect_reach = stats != nullptr && problem.packed_labels;
      // wide pending sets are expanded nearest half first (clients.hxx, select_near): where the label
      // scan exists and the run ends by itself on one GPU; GRX_SSSP_NEAR=0 switches it off
      problem.near_far = env_flag("GRX_SSSP_NEAR", true) && problem.packed_labels &&
                         lb == operators::load_balance_t::block_mapped && !o.call_every_edge &&
                         !o.holes_layout && o.max_iterations == 0 && !ctx->mc->communicator().attached() &&
                         (unsigned long long)G.get_number_of_edges() < (1ull << 32);
      problem.init();
      problem.reset();
      enactor_properties_t props;
      if (o.frontier_sizing_factor > 0)
        props.frontier_sizing_factor = o.frontier_sizing_factor;
      enactor_type enactor(&problem, ctx->mc, props);
      enactor.max_iterations = o.max_iterations;
      enactor.two_pass = o.sssp_two_pass != 0;
      enactor.bound_filter = env_flag("GRX_SSSP_BOUND_FILTER", o.call_every_edge == 0);
      enactor.early_live = env_flag("GRX_SSSP_EARLY_LIVE", enactor.early_live);
      enactor.bound_from = (int)env_or("GRX_SSSP_BOUND_FROM", enactor.bound_from, INT_MIN, INT_MAX);
      if (const char* e = std::getenv("GRX_SSSP_NEAR_FRAC"))  // for the sweep behind the default
        enactor.near_frac = std::min(1.0, std::max(1.0 / 64, std::atof(e)));
      const float ms = enactor.enact();
      if (stats) {
        run_stats(stats, ms, enactor.iteration, ctx->single());
        level_stats(stats, problem.log);
        // the first frontier ({source}) carries no work hint: add the source's own degree
        const unsigned long long* facts = ctx->single().workspace().run_facts();
        if (problem.collect_reach && facts[3] == 1ull) {  // left in pinned memory by unpack()
          stats->vertices_reached = (int64_t)facts[1];
          stats->edges_traversed = (int64_t)facts[2];
          stats->edges_expanded = problem.log.edges_expanded + (long long)facts[0];
        } else {
          stats->edges_expanded =
              problem.log.edges_expanded + reach_stats(g, d_distances, FLT_MAX, source, ctx->single(), stats);
        }
      }
      return (int)GRX_OK;
    });
  });
}

/** @file capi_cc.hip  grx_cc: connected components (weakly connected on a directed CSR) by Afforest
 * -- lock-free union-find on the output array, neighbour rounds, and a remainder pass that leaves the
 * rows of the picked component unread when the CSR is known to be symmetric
 * (hip/kernels/cc_kernels.hxx).  No reference counterpart.  One batch of launches, one hand-off. */
#include "capi_batch.hxx"

#include <gunrock/hip/kernels/cc_kernels.hxx>

#include <cstring>

using namespace essentials_amd;

namespace k = gunrock::hip::kernels;

extern "C" int grx_cc(grx_context_t ctx, grx_graph_t g, int32_t* d_component, int64_t* h_components,
                      const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_cc: NULL argument");
  if (!d_component && !h_components)
    return invalid("grx_cc: both outputs are NULL");
  if (g->n_rows != g->n_cols)
    return invalid("grx_cc: the graph is not square (n_rows != n_cols)");
  if (opt && opt->max_iterations != 0)
    return invalid("grx_cc: max_iterations must be 0 (the passes are fixed by the schedule)");
  const bool timed = opt && opt->collect_kernel_time;
  return guarded([&] {
    const int32_t n = g->n_rows;
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (h_components)
      *h_components = 0;
    if (n == 0)  // the empty graph: nothing to write
      return (int)GRX_OK;
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();

    // test hooks: the neighbour rounds (0 = hook every entry, leave no row out), and the entries
    // left above which a row is cut into segments for whole workgroups
    const int32_t rounds = (int32_t)env_or("GRX_CC_SAMPLE_ROUNDS", k::CC_SAMPLE_ROUNDS, 0, k::CC_MAX_ROUNDS);
    const int32_t big_row = (int32_t)env_or("GRX_CC_BIG_ROW", k::CC_BIG_ROW, 1, INT32_MAX);
    // a row of the picked component may stay unread only when its entries are stored from the other
    // end too: the handle's verdict as it stands (verifying it costs more than the whole call)
    const bool skip = rounds > 0 && !g->in_edges && g->symmetry == grx_graph_s::symmetric;

    call_clock_t clock(s, timed);
    clock.start();

    int32_t launches = 0;
    unsigned long long edges = 0, components = 0;
    {
      hip::device_array_t<int32_t> own_parent(d_component ? 0 : (std::size_t)n);
      hip::device_array_t<int2> big((std::size_t)(g->nnz / k::CC_BIG_SEGMENT) + (std::size_t)(g->nnz / big_row) + 1);
      hip::device_array_t<k::cc_counters_t> counters(1);
      int32_t* parent = d_component ? d_component : own_parent.data();
      k::cc_counters_t* ctr = counters.data();
      GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof *ctr, s));

      const unsigned grid = grid_for((std::size_t)n, k::CC_BLOCK, sc);

      clock.begin_batch();
      k::cc_init_kernel<<<grid, k::CC_BLOCK, 0, s>>>(parent, n);
      ++launches;
      for (int32_t r = 0; r < rounds; ++r) {
        k::cc_sample_kernel<<<grid, k::CC_BLOCK, 0, s>>>(g->d_ap, g->d_aj, parent, n, r, ctr);
        k::cc_compress_kernel<false><<<grid, k::CC_BLOCK, 0, s>>>(parent, n, ctr);
        launches += 2;
      }
      if (skip) {
        k::cc_pick_kernel<<<1, k::CC_SAMPLES, 0, s>>>(parent, n, ctr);
        ++launches;
      }
      k::cc_remainder_kernel<<<grid, k::CC_BLOCK, 0, s>>>(g->d_ap, g->d_aj, parent, n, rounds, skip ? 1 : 0, big_row,
                                                         big.data(), ctr);
      k::cc_big_kernel<<<(unsigned)sc.compute_units() * 4, k::CC_BLOCK, 0, s>>>(g->d_ap, g->d_aj, parent, rounds, big.data(),
                                                                              ctr);
      k::cc_compress_kernel<true><<<grid, k::CC_BLOCK, 0, s>>>(parent, n, ctr);
      launches += 4;
      // the one hand-off of the call
      const unsigned long long* m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
        k::cc_publish_kernel<<<1, 64, 0, s>>>(ctr, mirror, slot, seq);
      });
      edges = m[k::CC_EDGES];
      components = m[k::CC_COMPONENTS];
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();

    if (h_components)
      *h_components = (int64_t)components;
    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->iterations = rounds + 1;
      stats->advance_launches = launches;
      stats->vertices_reached = (int64_t)n - (int64_t)components;
      stats->edges_traversed = (int64_t)edges;
      stats->edges_expanded = (int64_t)edges;
    }
    return (int)GRX_OK;
  });
}

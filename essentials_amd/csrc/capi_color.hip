/** @file capi_color.hip  grx_color: greedy colouring in largest-degree-first order by
 * Jones-Plassmann (hip/kernels/color_kernels.hxx): one pass counts every vertex's predecessors, then
 * generation by generation the vertices without an uncoloured predecessor take the smallest absent
 * colour and tell the vertices they precede.  Each batch of launches ends with the one-workgroup
 * kernel, which runs the small generations itself and hands the counters over. */
#include "capi_batch.hxx"

#include <gunrock/hip/kernels/color_kernels.hxx>

using namespace essentials_amd;

namespace k = gunrock::hip::kernels;

extern "C" int grx_color(grx_context_t ctx, grx_graph_t g, int32_t* d_colors, int32_t* h_num_colors,
                         const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_color: NULL argument");
  if (!d_colors && !h_num_colors)
    return invalid("grx_color: both outputs are NULL");
  if (g->n_rows != g->n_cols)
    return invalid("grx_color: the graph is not square (n_rows != n_cols)");
  if (opt && opt->max_iterations != 0)
    return invalid("grx_color: max_iterations must be 0 (the colouring runs until every vertex has a colour)");
  const bool timed = opt && opt->collect_kernel_time;
  return guarded([&] {
    const int32_t n = g->n_rows;
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (h_num_colors)
      *h_num_colors = 0;
    if (n == 0)  // the empty graph: nothing to write
      return (int)GRX_OK;
    if (int rc = require_symmetric(ctx, g, "grx_color", "graph colouring"))
      return rc;
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();

    // test hooks: the entries a generation may have to stay in the one-workgroup kernel (0 sends
    // every generation to the wide kernel), the row length above which a row gets a workgroup of
    // its own, and the colours per LDS window of the smallest-absent-colour search
    const unsigned long long narrow_edges =
        (unsigned long long)env_or("GRX_COLOR_NARROW_EDGES", k::COLOR_NARROW_EDGES, 0, 1ll << 30);
    const int32_t narrow_vertices = narrow_edges ? k::COLOR_NARROW_BLOCK : 0;
    const int32_t big_row = (int32_t)env_or("GRX_COLOR_BIG_ROW", k::COLOR_BIG_ROW, 1, INT32_MAX);
    const int32_t window = (int32_t)env_or("GRX_COLOR_MEX_WINDOW", k::COLOR_MEX_WINDOW, 32, k::COLOR_MEX_WINDOW) / 32 * 32;

    call_clock_t clock(s, timed);
    clock.start();

    int32_t launches = 0;
    unsigned long long edges = 0, nonempty = 0, generations = 0, max_color = 0;
    {
      const std::size_t nnz = (std::size_t)g->nnz;
      hip::device_array_t<int32_t> pending((std::size_t)n), queue((std::size_t)n);
      hip::device_array_t<int32_t> own_colors(d_colors ? 0 : (std::size_t)n);
      hip::device_array_t<int32_t> big(nnz / big_row + 1);
      hip::device_array_t<int2> segments(nnz / k::COLOR_BIG_SEGMENT + nnz / big_row + 1);
      hip::device_array_t<k::color_counters_t> counters(1);
      int32_t* color = d_colors ? d_colors : own_colors.data();
      k::color_counters_t* ctr = counters.data();
      GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof *ctr, s));

      const unsigned most = (unsigned)sc.compute_units() * 8;
      // the hand-off that ends a batch is the narrow kernel's last act
      unsigned long long* m = nullptr;
      auto narrow = [&] {
        m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
          k::color_narrow_kernel<<<1, k::COLOR_NARROW_BLOCK, 0, s>>>(g->d_ap, g->d_aj, pending.data(), color,
                                                                    queue.data(), n, narrow_vertices, narrow_edges,
                                                                    window, ctr, mirror, slot, seq);
        });
        ++launches;
      };

      clock.begin_batch();
      k::color_init_kernel<<<grid_for((std::size_t)n, k::COLOR_BLOCK, sc), k::COLOR_BLOCK, 0, s>>>(
          g->d_ap, g->d_aj, n, big_row, pending.data(), color, queue.data(), segments.data(), ctr);
      k::color_init_big_kernel<<<most, k::COLOR_BLOCK, 0, s>>>(g->d_ap, g->d_aj, pending.data(), segments.data(), ctr);
      k::color_ready_kernel<<<1, k::COLOR_NARROW_BLOCK, 0, s>>>(g->d_ap, pending.data(), queue.data(), n,
                                                               segments.data(), ctr);
      launches += 3;
      narrow();
      const bool has_big = m[k::GQ_MAX_ROW] > (unsigned long long)big_row;
      generations = (unsigned long long)run_generations(
          sc, clock, m, k::COLOR_BLOCK, has_big, launches,
          [&](int32_t head, int32_t tail, int32_t chunk, unsigned grid) {
            k::color_wide_kernel<<<grid, k::COLOR_BLOCK, 0, s>>>(g->d_ap, g->d_aj, pending.data(), color, queue.data(), n,
                                                                head, tail, chunk, big_row, big.data(), window, ctr);
          },
          [&](unsigned grid) {
            k::color_big_kernel<<<grid, k::COLOR_BLOCK, 0, s>>>(g->d_ap, g->d_aj, pending.data(), color, queue.data(), n,
                                                               big.data(), window, ctr);
          },
          narrow);
      generations += m[k::CL_GENERATIONS];
      edges = m[k::GQ_EDGES];
      nonempty = m[k::GQ_NONEMPTY];
      max_color = m[k::CL_MAX_COLOR];
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();

    if (h_num_colors)
      *h_num_colors = (int32_t)max_color + 1;
    queue_call_stats(stats, clock, (int32_t)generations, launches, nonempty, (int64_t)g->nnz, edges);
    return (int)GRX_OK;
  });
}

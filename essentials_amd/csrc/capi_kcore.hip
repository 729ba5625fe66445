/** @file capi_kcore.hip  grx_kcore == gunrock::kcore::run (reference algorithms/kcore.hxx) by peeling:
 * per level one seed scan, then removal rounds until the queue is empty, every row walked once
 * when its vertex leaves (hip/kernels/kcore_kernels.hxx).  Each batch of launches ends with the
 * one-workgroup kernel, which runs the small generations itself and hands the counters over. */
#include "capi_batch.hxx"

#include <gunrock/hip/kernels/kcore_kernels.hxx>

using namespace essentials_amd;

namespace k = gunrock::hip::kernels;

extern "C" int grx_kcore(grx_context_t ctx, grx_graph_t g, int32_t* d_core, int32_t* h_degeneracy,
                         const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_kcore: NULL argument");
  if (!d_core && !h_degeneracy)
    return invalid("grx_kcore: both outputs are NULL");
  if (g->n_rows != g->n_cols)
    return invalid("grx_kcore: the graph is not square (n_rows != n_cols)");
  if (opt && opt->max_iterations != 0)
    return invalid("grx_kcore: max_iterations must be 0 (the peel runs until no vertex is left)");
  const bool timed = opt && opt->collect_kernel_time;
  return guarded([&] {
    const int32_t n = g->n_rows;
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (h_degeneracy)
      *h_degeneracy = 0;
    if (n == 0)  // the empty graph: nothing to write
      return (int)GRX_OK;
    if (int rc = require_symmetric(ctx, g, "grx_kcore", "k-core decomposition"))
      return rc;
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();

    // test hooks: the entries a generation may have to stay in the one-workgroup kernel (0 sends
    // every generation to the wide kernel), and the row length above which the whole grid walks a row
    const unsigned long long narrow_edges =
        (unsigned long long)env_or("GRX_KCORE_NARROW_EDGES", k::KCORE_NARROW_EDGES, 0, 1ll << 30);
    const int32_t big_row = (int32_t)env_or("GRX_KCORE_BIG_ROW", k::KCORE_BIG_ROW, 1, INT32_MAX);

    call_clock_t clock(s, timed);
    clock.start();

    int32_t degeneracy = 0, levels = 0, launches = 0;
    unsigned long long edges = 0, nonempty = 0;
    {
      hip::device_array_t<int32_t> deg((std::size_t)n), queue((std::size_t)n);
      hip::device_array_t<int32_t> own_core(d_core ? 0 : (std::size_t)n);
      hip::device_array_t<int32_t> big((std::size_t)(g->nnz / big_row) + 1);
      hip::device_array_t<k::kcore_counters_t> counters(1);
      int32_t* core = d_core ? d_core : own_core.data();
      k::kcore_counters_t* ctr = counters.data();
      GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof *ctr, s));
      GRX_HIP_CHECK(hipMemsetAsync(&ctr->next_k, 0xff, sizeof ctr->next_k, s));  // KCORE_NONE

      const unsigned scan_grid = grid_for((std::size_t)n, k::KCORE_BLOCK, sc);
      // the hand-off that ends a batch is the narrow kernel's last act
      unsigned long long* m = nullptr;
      auto narrow = [&](int32_t level) {
        m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
          k::kcore_narrow_kernel<<<1, k::KCORE_NARROW_BLOCK, 0, s>>>(g->d_ap, g->d_aj, deg.data(), core, queue.data(),
                                                                    n, level, k::KCORE_NARROW_BLOCK, narrow_edges, ctr,
                                                                    mirror, slot, seq);
        });
        ++launches;
      };

      clock.begin_batch();
      k::kcore_init_kernel<<<scan_grid, k::KCORE_BLOCK, 0, s>>>(g->d_ap, n, deg.data(), core, ctr);
      m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
        k::kcore_publish_kernel<<<1, 64, 0, s>>>(ctr, mirror, slot, seq);
      });
      launches += 2;
      const bool has_big = m[k::GQ_MAX_ROW] > (unsigned long long)big_row;
      nonempty = m[k::GQ_NONEMPTY];
      int32_t k_prev = 0;
      // each level removes at least the vertex whose degree named it
      while ((unsigned)m[k::KC_NEXT_K] != k::KCORE_NONE) {
        const int32_t level = (int32_t)m[k::KC_NEXT_K];
        const unsigned long long queued_before = m[k::GQ_TAIL];
        clock.begin_batch();
        k::kcore_seed_kernel<<<scan_grid, k::KCORE_BLOCK, 0, s>>>(g->d_ap, deg.data(), n, k_prev, level, queue.data(), ctr);
        ++launches;
        narrow(level);
        run_generations(
            sc, clock, m, k::KCORE_BLOCK, has_big, launches,
            [&](int32_t head, int32_t tail, int32_t chunk, unsigned grid) {
              k::kcore_wide_kernel<<<grid, k::KCORE_BLOCK, 0, s>>>(g->d_ap, g->d_aj, deg.data(), core, queue.data(), n, head,
                                                                  tail, chunk, level, big_row, big.data(), ctr);
            },
            [&](unsigned grid) {
              k::kcore_big_kernel<<<grid, k::KCORE_BLOCK, 0, s>>>(g->d_ap, g->d_aj, deg.data(), queue.data(), n, level,
                                                                 big.data(), ctr);
            },
            [&] { narrow(level); });
        k_prev = level;
        // the seed scan's smallest degree above k may belong to a vertex that left later in that
        // level: then nobody has this degree, the level is empty and names the next one exactly
        if (m[k::GQ_TAIL] > queued_before) {
          ++levels;
          degeneracy = level;
        }
      }
      edges = m[k::GQ_EDGES];
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();

    if (h_degeneracy)
      *h_degeneracy = degeneracy;
    queue_call_stats(stats, clock, levels, launches, nonempty, (int64_t)edges, edges);
    return (int)GRX_OK;
  });
}

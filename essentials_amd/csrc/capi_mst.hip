/** @file capi_mst.hip  grx_mst: minimum spanning forest of the CSR as given by Boruvka rounds on a
 * flat component array -- every row entry an undirected candidate, strictly ordered by
 * (ordered_bits(weight), position) (hip/kernels/mst_kernels.hxx).  The reference's mst.hxx returns one
 * order-dependent float on connected graphs only; this returns the entries, an exact count, a
 * reproducible float64 weight and the component labels, on any graph.  One hand-off per round + one. */
#include "capi_batch.hxx"

#include <gunrock/hip/kernels/mst_kernels.hxx>

#include <cstring>

using namespace essentials_amd;

namespace {

namespace k = gunrock::hip::kernels;

/// ceil(log2(x)) for x >= 1.
int ceil_log2(unsigned long long x) {
  int b = 0;
  while ((1ull << b) < x)
    ++b;
  return b;
}

}  // namespace

extern "C" int grx_mst(grx_context_t ctx, grx_graph_t g, int32_t* d_entries, int64_t* h_count, double* h_weight,
                       int32_t* d_component, const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_mst: NULL argument");
  if (!d_entries && !h_count && !h_weight && !d_component)
    return invalid("grx_mst: every output is NULL");
  if (g->n_rows != g->n_cols)
    return invalid("grx_mst: the graph is not square (n_rows != n_cols)");
  if (opt && opt->max_iterations != 0)
    return invalid("grx_mst: max_iterations must be 0 (the rounds are fixed by the schedule)");
  const bool timed = opt && opt->collect_kernel_time;
  return guarded([&] {
    const int32_t n = g->n_rows;
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (h_count)
      *h_count = 0;
    if (h_weight)
      *h_weight = 0.0;
    if (n == 0)  // the empty graph: nothing to write
      return (int)GRX_OK;
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();

    // test hooks: the entries above which a row is cut into segments for whole workgroups, and the
    // row flags (1: a row whose entries are all inside one component is flagged and not walked
    // again; 0: every row is walked in every round)
    const int32_t big_row = (int32_t)env_or("GRX_MST_BIG_ROW", k::MST_BIG_ROW, 1, INT32_MAX);
    const int use_flags = (int)env_or("GRX_MST_ROW_FLAGS", 1, 0, 1);

    call_clock_t clock(s, timed);
    clock.start();

    int32_t launches = 0, rounds = 0;
    unsigned long long edges = 0, count = 0;
    double weight = 0.0;
    {
      const int64_t nnz = g->nnz;
      const int64_t words = (nnz + 31) / 32, tiles = (words + k::MST_BLOCK - 1) / k::MST_BLOCK;
      // the whole workspace of the call, before the first round
      hip::device_array_t<int32_t> comp((std::size_t)n), link((std::size_t)n);
      hip::device_array_t<unsigned long long> best((std::size_t)n);
      hip::device_array_t<unsigned char> done((std::size_t)n);
      hip::device_array_t<unsigned int> chosen((std::size_t)std::max<int64_t>(words, 1));
      hip::device_array_t<unsigned int> tile_count((std::size_t)std::max<int64_t>(tiles, 1));
      hip::device_array_t<double> tile_sum((std::size_t)std::max<int64_t>(tiles, 1));
      hip::device_array_t<int2> big((std::size_t)(nnz / k::MST_BIG_SEGMENT) + (std::size_t)(nnz / big_row) + 1);
      hip::device_array_t<k::mst_counters_t> counters(1);
      k::mst_counters_t* ctr = counters.data();
      GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof *ctr, s));
      GRX_HIP_CHECK(hipMemsetAsync(chosen.data(), 0, (std::size_t)std::max<int64_t>(words, 1) * sizeof(unsigned int), s));

      const unsigned grid = grid_for((std::size_t)n, k::MST_BLOCK, sc);
      const unsigned tile_grid = grid_for((std::size_t)tiles, 1, sc);

      // the hand-off that ends a batch of launches
      auto publish = [&](unsigned long long* mirror, int slot, unsigned long long seq) {
        k::mst_publish_kernel<<<1, 64, 0, s>>>(ctr, mirror, slot, seq);
        ++launches;
      };

      clock.begin_batch();
      k::mst_init_kernel<<<grid, k::MST_BLOCK, 0, s>>>(comp.data(), best.data(), done.data(), n);
      ++launches;
      // Components that can still grow: one that did not merge in a round has no outgoing entry and
      // never will, so after a round with h hooks at most h components are live -- a bound on the
      // depth of the next round's hooking trees (pointer-jumping passes) and on the rounds left.
      unsigned long long live = (unsigned long long)n;
      while (nnz > 0 && live > 1) {
        if (rounds)
          clock.begin_batch();
        k::mst_search_kernel<<<grid, k::MST_BLOCK, 0, s>>>(g->d_ap, g->d_aj, g->d_ax, comp.data(), best.data(), done.data(), n,
                                                         use_flags, big_row, big.data(), ctr);
        k::mst_big_kernel<<<(unsigned)sc.compute_units() * 4, k::MST_BLOCK, 0, s>>>(g->d_ap, g->d_aj, g->d_ax, comp.data(),
                                                                                 best.data(), done.data(), use_flags,
                                                                                 big.data(), ctr);
        k::mst_hook_kernel<<<grid, k::MST_BLOCK, 0, s>>>(g->d_ap, g->d_aj, comp.data(), best.data(), link.data(),
                                                       chosen.data(), n, ctr);
        const int jumps = std::min(k::MST_MAX_JUMPS, std::max(1, ceil_log2(live)));
        for (int j = 0; j < jumps; ++j)
          k::mst_jump_kernel<<<grid, k::MST_BLOCK, 0, s>>>(comp.data(), link.data(), n, j, ctr);
        k::mst_flatten_kernel<<<grid, k::MST_BLOCK, 0, s>>>(comp.data(), link.data(), best.data(), n);
        launches += 4 + jumps;
        ++rounds;
        const unsigned long long* m = hand_off(sc, clock, publish);
        edges = m[k::MST_EDGES];
        live = m[k::MST_HOOKED];
      }

      // the last batch: labels, the chosen positions in ascending order, their weights' sum
      if (rounds)
        clock.begin_batch();
      if (d_component) {
        k::mst_minid_init_kernel<<<grid, k::MST_BLOCK, 0, s>>>(link.data(), n);
        k::mst_minid_kernel<<<grid, k::MST_BLOCK, 0, s>>>(comp.data(), link.data(), n);
        k::mst_label_kernel<<<grid, k::MST_BLOCK, 0, s>>>(comp.data(), link.data(), d_component, n);
        launches += 3;
      }
      if (nnz > 0) {
        k::mst_tile_count_kernel<<<tile_grid, k::MST_BLOCK, 0, s>>>(chosen.data(), words, tiles, tile_count.data());
        k::mst_tile_scan_kernel<<<1, k::MST_SCAN_BLOCK, 0, s>>>(tile_count.data(), tiles, ctr);
        k::mst_emit_kernel<<<tile_grid, k::MST_BLOCK, 0, s>>>(chosen.data(), g->d_ax, words, tiles, tile_count.data(),
                                                            d_entries, (int64_t)n, tile_sum.data());
        k::mst_sum_kernel<<<1, k::MST_SCAN_BLOCK, 0, s>>>(tile_sum.data(), tiles, ctr);
        launches += 4;
      }
      const unsigned long long* m = hand_off(sc, clock, publish);
      count = m[k::MST_COUNT];
      const long long bits = (long long)m[k::MST_WEIGHT];
      std::memcpy(&weight, &bits, sizeof weight);
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();

    if (h_count)
      *h_count = (int64_t)count;
    if (h_weight)
      *h_weight = weight;
    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->iterations = rounds;
      stats->advance_launches = launches;
      stats->vertices_reached = (int64_t)count;
      stats->edges_traversed = (int64_t)edges;
      stats->edges_expanded = (int64_t)edges;
    }
    return (int)GRX_OK;
  });
}

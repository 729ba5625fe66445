/** @file capi_scc.hip  grx_scc: strongly connected components by forward-backward with trimming, all
 * regions at once (hip/kernels/scc_kernels.hxx).  No reference counterpart.  A round is four
 * phases on one generation queue: count the alive entries and trim, pick a pivot per region and
 * reach forwards over the out-rows, reach backwards over the in-rows, then finish FW n BW and rename
 * the remainders (those two kernels open the next round's batch).  Each batch of launches ends with
 * the one-workgroup kernel, which runs the small generations itself and hands the counters over. */
#include "capi_batch.hxx"

#include <gunrock/hip/kernels/scc_kernels.hxx>

using namespace essentials_amd;

namespace k = gunrock::hip::kernels;

extern "C" int grx_scc(grx_context_t ctx, grx_graph_t g, int32_t* d_component, int64_t* h_components,
                       const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_scc: NULL argument");
  if (!d_component && !h_components)
    return invalid("grx_scc: both outputs are NULL");
  if (g->n_rows != g->n_cols)
    return invalid("grx_scc: the graph is not square (n_rows != n_cols)");
  if (opt && opt->max_iterations != 0)
    return invalid("grx_scc: max_iterations must be 0 (the rounds run until every vertex has a component)");
  const bool timed = opt && opt->collect_kernel_time;
  bool undirected = false;
  const int rc = guarded([&] {
    const int32_t n = g->n_rows;
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (h_components)
      *h_components = 0;
    if (n == 0)  // the empty graph: nothing to write
      return (int)GRX_OK;
    if (!g->in_edges) {
      // no transpose: only a CSR that is its own transpose can be answered, and the answer is grx_cc's
      if (ensure_can_pull(ctx, g) != GRX_OK)
        return unsupported(
            "grx_scc: the CSR is not symmetric (directed) and has no in-edges; attach them with "
            "grx_graph_build_in_edges");
      undirected = true;
      return (int)GRX_OK;
    }
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();

    // test hooks: the row length above which the whole grid walks a row, the entries a generation
    // may have to stay in the one-workgroup kernel (0 sends every generation to the wide kernel),
    // and whether vertices without an alive out- or in-entry are trimmed (0: they end as pivots)
    const int32_t big_row = (int32_t)env_or("GRX_SCC_BIG_ROW", k::SCC_BIG_ROW, 1, INT32_MAX);
    const unsigned long long narrow_edges =
        (unsigned long long)env_or("GRX_SCC_NARROW_EDGES", k::SCC_NARROW_EDGES, 0, 1ll << 30);
    const int32_t narrow_vertices = narrow_edges ? k::SCC_NARROW_BLOCK : 0;
    const bool trim = env_or("GRX_SCC_TRIM", 1, 0, 1) != 0;

    call_clock_t clock(s, timed);
    clock.start();

    int32_t rounds = 0, launches = 0;
    unsigned long long edges = 0, trimmed = 0, pivots = 0;
    {
      const std::size_t nnz = (std::size_t)g->nnz;
      hip::device_array_t<k::scc_state_t> st((std::size_t)n);
      hip::device_array_t<unsigned long long> table((std::size_t)3 * (std::size_t)n + 1);
      hip::device_array_t<int32_t> out_cnt((std::size_t)n), in_cnt((std::size_t)n), queue((std::size_t)n);
      hip::device_array_t<int32_t> own_label(d_component ? 0 : (std::size_t)n);
      hip::device_array_t<int32_t> big_out(nnz / big_row + 1), big_in(nnz / big_row + 1);
      hip::device_array_t<int2> segments(2 * (nnz / k::SCC_BIG_SEGMENT + nnz / big_row + 1));
      hip::device_array_t<k::scc_counters_t> counters(1);
      int32_t* label = d_component ? d_component : own_label.data();
      k::scc_counters_t* ctr = counters.data();
      GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof *ctr, s));
      GRX_HIP_CHECK(hipMemsetAsync(st.data(), 0, sizeof(k::scc_state_t) * (std::size_t)n, s));
      GRX_HIP_CHECK(hipMemsetAsync(table.data(), 0, sizeof(unsigned long long) * ((std::size_t)3 * (std::size_t)n + 1), s));

      const k::scc_rows_t out{g->d_ap, g->d_aj}, in{g->in_edges->offsets.data(), g->in_edges->indices.data()};
      auto pass_over = [&](const k::scc_rows_t& a, const k::scc_rows_t& b, k::scc_state_t bit) {
        return k::scc_pass_t{a,     b,       bit,            st.data(),    out_cnt.data(), in_cnt.data(),
                             label, big_row, big_out.data(), big_in.data()};
      };
      const k::scc_pass_t trim_pass = pass_over(out, in, 0), forward = pass_over(out, in, k::SCC_FW),
                          backward = pass_over(in, out, k::SCC_BW);

      const unsigned scan_grid = grid_for((std::size_t)n, k::SCC_BLOCK, sc);
      const unsigned most = (unsigned)sc.compute_units() * 8;
      bool has_big = true;  // until the first hand-off names the longest row
      unsigned long long* m = nullptr;
      // a phase starts the queue afresh: every vertex enters it at most once per phase
      auto restart_queue = [&] { GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, 2 * sizeof(int), s)); };
      // the generations of one phase; the hand-off that ends a batch is the narrow kernel's last act
      auto run_phase = [&](auto is_trim, const k::scc_pass_t& pass, auto&& after_first) {
        constexpr bool TRIM = decltype(is_trim)::value;
        auto narrow = [&] {
          m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
            k::scc_narrow_kernel<TRIM><<<1, k::SCC_NARROW_BLOCK, 0, s>>>(pass, queue.data(), n, narrow_vertices,
                                                                        narrow_edges, ctr, mirror, slot, seq);
          });
          ++launches;
        };
        narrow();
        after_first();
        run_generations(
            sc, clock, m, k::SCC_BLOCK, has_big, launches,
            [&](int32_t head, int32_t tail, int32_t chunk, unsigned grid) {
              k::scc_wide_kernel<TRIM><<<grid, k::SCC_BLOCK, 0, s>>>(pass, queue.data(), n, head, tail, chunk, ctr);
            },
            [&](unsigned grid) { k::scc_big_kernel<TRIM><<<grid, k::SCC_BLOCK, 0, s>>>(pass, queue.data(), n, ctr); },
            narrow);
      };

      for (;;) {
        // count the alive entries of what is left and trim
        clock.begin_batch();
        if (rounds > 0) {  // the round before: FW n BW is finished, the remainders are the new regions
          k::scc_min_kernel<<<scan_grid, k::SCC_BLOCK, 0, s>>>(st.data(), n, table.data(), label);
          k::scc_finish_kernel<<<scan_grid, k::SCC_BLOCK, 0, s>>>(st.data(), n, table.data(), label, ctr);
          launches += 2;
        }
        restart_queue();
        k::scc_count_kernel<<<scan_grid, k::SCC_BLOCK, 0, s>>>(out, in, st.data(), n, big_row, out_cnt.data(),
                                                              in_cnt.data(), segments.data(), ctr);
        ++launches;
        if (has_big) {
          k::scc_count_big_kernel<<<most, k::SCC_BLOCK, 0, s>>>(out, in, st.data(), out_cnt.data(), in_cnt.data(),
                                                               segments.data(), ctr);
          ++launches;
        }
        if (trim) {
          k::scc_trim_seed_kernel<<<scan_grid, k::SCC_BLOCK, 0, s>>>(out.ap, in.ap, st.data(), out_cnt.data(),
                                                                    in_cnt.data(), n, queue.data(), ctr);
          ++launches;
        }
        run_phase(std::true_type{}, trim_pass, [&] { has_big = m[k::GQ_MAX_ROW] > (unsigned long long)big_row; });
        trimmed += m[k::GQ_TAIL];  // the phase's queue started at 0
        if (trimmed + m[k::SC_FINISHED] >= (unsigned long long)n)
          break;
        // every round finishes its pivots, so V rounds finish everything; more is a fault, not a spin
        error::throw_if_exception(rounds >= n, "grx_scc: more forward-backward rounds than vertices");
        ++rounds;

        // a pivot per region, and what it reaches along the out-rows
        clock.begin_batch();
        restart_queue();
        k::scc_pivot_max_kernel<<<scan_grid, k::SCC_BLOCK, 0, s>>>(st.data(), out_cnt.data(), in_cnt.data(), n,
                                                                  table.data());
        k::scc_pivot_seed_kernel<<<scan_grid, k::SCC_BLOCK, 0, s>>>(out.ap, in.ap, st.data(), out_cnt.data(),
                                                                   in_cnt.data(), n, table.data(), label, queue.data(),
                                                                   ctr);
        launches += 2;
        unsigned long long seeds = 0, seed_in = 0;
        run_phase(std::false_type{}, forward, [&] {
          seeds = m[k::SC_SEEDS];
          seed_in = m[k::SC_SEED_IN];
        });
        error::throw_if_exception(seeds == 0, "grx_scc: a round without a pivot");
        pivots += seeds;

        // ... and what reaches it, along the in-rows
        clock.begin_batch();
        k::scc_rewind_kernel<<<1, 64, 0, s>>>(ctr, (int)seeds, seed_in);
        ++launches;
        run_phase(std::false_type{}, backward, [] {});
      }
      edges = m[k::GQ_EDGES];
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();

    const unsigned long long components = trimmed + pivots;
    if (h_components)
      *h_components = (int64_t)components;
    queue_call_stats(stats, clock, rounds, launches, (unsigned long long)n - components, (int64_t)edges, edges);
    return (int)GRX_OK;
  });
  if (rc == GRX_OK && undirected)  // every edge runs both ways: the weak components are the strong ones
    return grx_cc(ctx, g, d_component, h_components, opt, stats);
  return rc;
}

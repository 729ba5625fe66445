/** @file capi_lpa.hip  grx_lpa: communities by semi-synchronous label propagation over the colour
 * classes of grx_color, and grx_modularity: the score of any labelling in exact integers
 * (hip/kernels/lpa_kernels.hxx).  No reference counterpart.  The schedule and the launches of a
 * sweep are capi_class_sweep.hxx, shared with grx_louvain; a sweep ends with the one hand-off that
 * carries its change count, and the sweeps stop when one changes nothing. */
#include "capi_class_sweep.hxx"

#include <gunrock/hip/kernels/lpa_kernels.hxx>

#include <cstring>

using namespace essentials_amd;

namespace {

namespace k = gunrock::hip::kernels;

/// Enqueue the modularity passes over `label`: the range check, tot, I and S land in `ctr`.  `tot`:
/// V words, zeroed here; `big`: big_list_size(nnz) items.  Returns the launches.
int32_t enqueue_modularity(gcuda::standard_context_t& sc, grx_graph_s* g, const int32_t* label, unsigned* tot,
                           int2* big, k::lpa_counters_t* ctr) {
  const hipStream_t s = sc.stream();
  const int32_t n = g->n_rows;
  const unsigned grid = grid_for((std::size_t)n, k::LPA_BLOCK, sc);
  GRX_HIP_CHECK(hipMemsetAsync(tot, 0, sizeof(unsigned) * (std::size_t)n, s));
  k::lpa_range_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(label, n, ctr);
  k::lpa_tot_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(g->d_ap, label, n, tot);
  const int32_t launches = 2 + enqueue_score<false>(sc, g->d_ap, g->d_aj, nullptr, label, n, tot, big, ctr);
  GRX_HIP_CHECK(hipGetLastError());
  return launches;
}

}  // namespace

extern "C" int grx_modularity(grx_context_t ctx, grx_graph_t g, const int32_t* d_label, double* h_modularity,
                              int64_t* h_inside_entries, uint64_t* h_degree_squares, const grx_options* opt,
                              grx_stats* stats) {
  if (!ctx || !g || (!d_label && g->n_rows > 0))  // the labels of no vertices may be nowhere
    return invalid("grx_modularity: NULL argument");
  if (!h_modularity && !h_inside_entries && !h_degree_squares)
    return invalid("grx_modularity: all three outputs are NULL");
  if (g->n_rows != g->n_cols)
    return invalid("grx_modularity: the graph is not square (n_rows != n_cols)");
  const bool timed = opt && opt->collect_kernel_time;
  return guarded([&] {
    const int32_t n = g->n_rows;
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    unsigned long long inside = 0, squares = 0;
    int32_t launches = 0;
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();
    call_clock_t clock(s, timed);
    clock.start();
    if (n > 0) {
      hip::device_array_t<unsigned> tot((std::size_t)n);
      hip::device_array_t<int2> big(big_list_size(g->nnz));
      hip::device_array_t<k::lpa_counters_t> counters(1);
      k::lpa_counters_t* ctr = counters.data();
      GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof *ctr, s));
      clock.begin_batch();
      launches += enqueue_modularity(sc, g, d_label, tot.data(), big.data(), ctr);
      const unsigned long long* m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
        k::lpa_publish_kernel<<<1, 64, 0, s>>>(ctr, mirror, slot, seq);
      });
      ++launches;
      const bool bad = m[k::LPA_BAD] != 0;
      inside = m[k::LPA_INSIDE];
      squares = m[k::LPA_SQUARES];
      clock.stop_and_wait();
      if (bad)
        return invalid("grx_modularity: a label is outside [0, V)");
    } else {
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();
    if (h_modularity)
      *h_modularity = modularity_of(inside, squares, g->nnz);
    if (h_inside_entries)
      *h_inside_entries = (int64_t)inside;
    if (h_degree_squares)
      *h_degree_squares = (uint64_t)squares;
    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->iterations = 1;
      stats->advance_launches = launches;
      stats->edges_traversed = g->nnz;
      stats->edges_expanded = g->nnz;
    }
    return (int)GRX_OK;
  });
}

extern "C" int grx_lpa(grx_context_t ctx, grx_graph_t g, int32_t* d_community, int64_t* h_communities,
                       double* h_modularity, const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_lpa: NULL argument");
  if (!d_community && !h_communities && !h_modularity)
    return invalid("grx_lpa: all three outputs are NULL");
  if (g->n_rows != g->n_cols)
    return invalid("grx_lpa: the graph is not square (n_rows != n_cols)");
  if (opt && opt->max_iterations < 0)
    return invalid("grx_lpa: max_iterations must not be negative");
  const bool timed = opt && opt->collect_kernel_time;
  const int32_t max_sweeps = opt ? opt->max_iterations : 0;
  return guarded([&] {
    const int32_t n = g->n_rows;
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (h_communities)
      *h_communities = 0;
    if (h_modularity)
      *h_modularity = 0.0;
    if (n == 0)  // the empty graph: nothing to write
      return (int)GRX_OK;
    if (int rc = require_symmetric(ctx, g, "grx_lpa", "label propagation"))
      return rc;
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();

    // test hooks: the three of the shared sweep, and whether every vertex decides every sweep
    const sweep_limits_t lim = sweep_limits("GRX_LPA");
    const bool all_rows = env_flag("GRX_LPA_ALL_ROWS", false);

    call_clock_t clock(s, timed);
    clock.start();

    int32_t launches = 0, sweeps = 0;
    unsigned long long read = 0, communities = 0, inside = 0, squares = 0;
    std::vector<unsigned long long> changed;
    {
      // 1. the colour classes, the vertices by (class, bin) and the launch plan of a sweep
      class_schedule_t sched;
      if (int rc = sched.build(ctx, g, g->d_ap, n, lim, clock, launches, "grx_lpa"))
        return rc;

      hip::device_array_t<int32_t> own_label(d_community ? 0 : (std::size_t)n);
      hip::device_array_t<unsigned char> dirty(all_rows ? 0 : (std::size_t)n);
      hip::device_array_t<unsigned> tot(h_modularity ? (std::size_t)n : 0);
      hip::device_array_t<int2> big(h_modularity ? big_list_size(g->nnz) : 0);
      hip::device_array_t<k::lpa_counters_t> counters(1);
      k::lpa_counters_t* ctr = counters.data();
      int32_t* label = d_community ? d_community : own_label.data();
      const k::lpa_state_t st{g->d_ap, g->d_aj, label, all_rows ? nullptr : dirty.data()};

      // 2. sweeps until one changes nothing
      GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof *ctr, s));
      clock.begin_batch();
      k::lpa_init_kernel<<<grid_for((std::size_t)n, k::LPA_BLOCK, sc), k::LPA_BLOCK, 0, s>>>(label, st.dirty, n);
      ++launches;
      const unsigned long long* m = nullptr;
      for (;;) {
        // every changing sweep raises the entries whose ends share a label by at least 2, and there
        // are nnz of them: more sweeps is a fault of the kernels, not a spin
        error::throw_if_exception((long long)sweeps >= (long long)g->nnz / 2 + 2,
                                  "grx_lpa: more sweeps than the entries allow");
        enqueue_sweep<k::lpa_decision_t>(sc, sched, st, ctr, launches);
        m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
          k::lpa_publish_kernel<<<1, 64, 0, s>>>(ctr, mirror, slot, seq);
        });
        ++launches;
        ++sweeps;
        changed.push_back(m[k::LPA_CHANGES]);
        read = m[k::LPA_READ];
        if (changed.back() == 0 || sweeps == max_sweeps)
          break;
        clock.begin_batch();
      }

      // 3. the smallest member names its community; the score of the result
      unsigned* first = sched.keys.data();  // the sorted keys are done with
      clock.begin_batch();
      GRX_HIP_CHECK(hipMemsetAsync(first, 0xff, sizeof(unsigned) * (std::size_t)n, s));
      const unsigned grid = grid_for((std::size_t)n, k::LPA_BLOCK, sc);
      k::lpa_first_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(label, n, first);
      k::lpa_canonical_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(label, n, first, ctr);
      launches += 2;
      if (h_modularity)
        launches += enqueue_modularity(sc, g, label, tot.data(), big.data(), ctr);
      m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
        k::lpa_publish_kernel<<<1, 64, 0, s>>>(ctr, mirror, slot, seq);
      });
      ++launches;
      communities = m[k::LPA_COMMUNITIES];
      inside = m[k::LPA_INSIDE];
      squares = m[k::LPA_SQUARES];
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();

    if (h_communities)
      *h_communities = (int64_t)communities;
    if (h_modularity)
      *h_modularity = modularity_of(inside, squares, g->nnz);
    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->iterations = sweeps;
      stats->advance_launches = launches;
      stats->vertices_reached = (int64_t)n - (int64_t)communities;
      stats->edges_traversed = g->nnz;
      stats->edges_expanded = (int64_t)read;
      stats->levels_recorded = std::min(sweeps, 64);
      for (int32_t t = 0; t < stats->levels_recorded; ++t)
        stats->frontier_slots[t] = (int64_t)changed[(std::size_t)t];
    }
    return (int)GRX_OK;
  });
}

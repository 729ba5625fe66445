/** @file capi_louvain.hip  grx_louvain: communities by multi-level modularity optimisation in exact
 * integers (hip/kernels/louvain_kernels.hxx; include/essentials_amd.h states the definition).  No
 * reference counterpart.  A phase builds the schedule of its level graph and sweeps it with the
 * launches of capi_class_sweep.hxx, shared with grx_lpa; every wide class is followed by its apply
 * launch, and a sweep ends with the score passes and the one hand-off that carries its moves, I
 * and S.  The communities of a phase that kept a move are contracted by a radix sort and a
 * reduction by key into the next level graph.  The workspace is released on return; the handle
 * keeps nothing but the symmetry verdict. */
#include "capi_class_sweep.hxx"

#include <gunrock/hip/kernels/louvain_kernels.hxx>

#include <cstring>

using namespace essentials_amd;

namespace {

namespace k = gunrock::hip::kernels;

/// A level graph: the caller's CSR on level 0 (no weights, no copy), arrays of its own above.
struct level_t {
  int32_t n = 0;
  int64_t entries = 0;
  const int32_t* ap = nullptr;
  const int32_t* aj = nullptr;
  const int32_t* aw = nullptr;
  hip::device_array_t<int32_t> own_ap, own_aj, own_aw;
  hip::device_array_t<int32_t> k;  // k(v); level 0: filled by the phase's init
};

/// What a call accumulates over its phases.
struct tally_t {
  int32_t launches = 0;
  int64_t expanded = 0;
  std::vector<int64_t> kept;  // per sweep
  unsigned long long inside = 0, squares = 0;
  bool scored = false;
};

long long score_of(unsigned long long inside, unsigned long long squares, int64_t entries) {
  return (long long)inside * (long long)entries - (long long)squares;
}

/// One phase on `lv`: label[] (level-local community per level vertex) and tot[] are filled.
/// Returns GRX_OK and sets `kept_any`.
template <bool W>
int run_phase(grx_context_s* ctx, grx_graph_s* pattern, level_t& lv, const sweep_limits_t& lim, int64_t E,
              call_clock_t& clock, tally_t& tally, hip::device_array_t<int32_t>& label_out,
              hip::device_array_t<int32_t>& tot_out, bool& kept_any) {
  auto& sc = ctx->single();
  const hipStream_t s = sc.stream();
  const int32_t n = lv.n;
  kept_any = false;

  // 1. the colour classes of the level's pattern CSR, the vertices by (class, bin) and the plan
  class_schedule_t sched;
  if (int rc = sched.build(ctx, pattern, lv.ap, n, lim, clock, tally.launches, "grx_louvain"))
    return rc;

  hip::device_array_t<int32_t> label((std::size_t)n), before((std::size_t)n), tot((std::size_t)n),
      tot_before((std::size_t)n);
  hip::device_array_t<int2> big(big_list_size(lv.entries));
  hip::device_array_t<k::louvain_counters_t> counters(1);
  k::louvain_counters_t* ctr = counters.data();
  if (!W)
    lv.k = hip::device_array_t<int32_t>((std::size_t)n);
  const k::louvain_state_t st{lv.ap, lv.aj, lv.aw, lv.k.data(), label.data(), before.data(), tot.data(), (long long)E};

  using decision_t = k::louvain_decision_t<W>;
  auto score = [&] {
    tally.launches += enqueue_score<W>(sc, lv.ap, lv.aj, lv.aw, label.data(), n, tot.data(), big.data(), ctr);
  };
  auto publish = [&](unsigned long long* mirror, int slot, unsigned long long seq) {
    k::louvain_publish_kernel<<<1, 64, 0, s>>>(ctr, mirror, slot, seq);
  };

  // 2. label[v] = v, tot[v] = k(v); the first phase scores that partition, the later ones inherit
  // the score: aggregation changes neither E nor N
  GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof *ctr, s));
  clock.begin_batch();
  k::louvain_init_kernel<W><<<grid_for((std::size_t)n, k::LPA_BLOCK, sc), k::LPA_BLOCK, 0, s>>>(
      lv.ap, lv.k.data(), label.data(), tot.data(), n);
  ++tally.launches;
  if (!tally.scored) {
    score();
    const unsigned long long* m = hand_off(sc, clock, publish);
    ++tally.launches;
    tally.inside = m[k::LOUVAIN_INSIDE];
    tally.squares = m[k::LOUVAIN_SQUARES];
    tally.scored = true;
    clock.begin_batch();
  }

  // 3. sweeps until one moves nothing or fails to raise the score
  const std::size_t bytes = sizeof(int32_t) * (std::size_t)n;
  for (int32_t sweeps = 0;; ++sweeps) {
    // N rises by at least 1 per kept sweep and is at most E^2: more is a fault of the kernels
    error::throw_if_exception(sweeps > 100000, "grx_louvain: more sweeps than a phase can keep");
    GRX_HIP_CHECK(hipMemcpyAsync(before.data(), label.data(), bytes, hipMemcpyDeviceToDevice, s));
    GRX_HIP_CHECK(hipMemcpyAsync(tot_before.data(), tot.data(), bytes, hipMemcpyDeviceToDevice, s));
    enqueue_sweep<decision_t>(sc, sched, st, ctr, tally.launches);
    score();
    const unsigned long long* m = hand_off(sc, clock, publish);
    ++tally.launches;
    tally.expanded += lv.entries;
    const unsigned long long moves = m[k::LOUVAIN_MOVES], inside = m[k::LOUVAIN_INSIDE], squares = m[k::LOUVAIN_SQUARES];
    if (moves == 0) {
      tally.kept.push_back(0);
      break;
    }
    if (score_of(inside, squares, E) <= score_of(tally.inside, tally.squares, E)) {  // undone
      GRX_HIP_CHECK(hipMemcpyAsync(label.data(), before.data(), bytes, hipMemcpyDeviceToDevice, s));
      GRX_HIP_CHECK(hipMemcpyAsync(tot.data(), tot_before.data(), bytes, hipMemcpyDeviceToDevice, s));
      tally.kept.push_back(0);
      break;
    }
    tally.inside = inside;
    tally.squares = squares;
    tally.kept.push_back((int64_t)moves);
    kept_any = true;
    clock.begin_batch();
  }
  GRX_HIP_CHECK(hipStreamSynchronize(s));  // the phase's workspace is released behind it
  label_out = std::move(label);
  tot_out = std::move(tot);
  return (int)GRX_OK;
}

/// The communities of `label` ranked by their smallest member: comm[] is composed with the new ids,
/// and when `build` the level graph contracted into `next`.  Returns the number of communities.
template <bool W>
int32_t aggregate(gcuda::standard_context_t& sc, const level_t& lv, const int32_t* label, const int32_t* tot,
                  int32_t* comm, int32_t n_original, bool build, level_t& next, tally_t& tally) {
  const hipStream_t s = sc.stream();
  const int32_t n = lv.n;
  const unsigned grid = grid_for((std::size_t)n, k::LPA_BLOCK, sc);
  hip::device_array_t<unsigned> first((std::size_t)n);
  hip::device_array_t<int32_t> flag((std::size_t)n), rank((std::size_t)n), nid((std::size_t)n);
  GRX_HIP_CHECK(hipMemsetAsync(first.data(), 0xff, sizeof(unsigned) * (std::size_t)n, s));
  k::lpa_first_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(label, n, first.data());
  k::louvain_flag_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(label, first.data(), n, flag.data());
  GRX_HIP_CHECK(hipGetLastError());
  {
    const std::size_t bytes = hip::exclusive_sum_temp_bytes(flag.data(), rank.data(), (int32_t)0, (std::size_t)n);
    hip::device_array_t<unsigned char> temp(std::max<std::size_t>(bytes, 256));
    hip::exclusive_sum(temp.data(), bytes, flag.data(), rank.data(), (int32_t)0, (std::size_t)n, s);
    int32_t last[2] = {0, 0};
    GRX_HIP_CHECK(hipMemcpyAsync(&last[0], rank.data() + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GRX_HIP_CHECK(hipMemcpyAsync(&last[1], flag.data() + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GRX_HIP_CHECK(hipStreamSynchronize(s));
    next.n = last[0] + last[1];
  }
  error::throw_if_exception(next.n <= 0 || next.n > n, "grx_louvain: the communities were miscounted");
  next.k = hip::device_array_t<int32_t>((std::size_t)next.n);
  k::louvain_renumber_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(label, first.data(), rank.data(), tot, n, nid.data(),
                                                           next.k.data());
  k::louvain_compose_kernel<<<grid_for((std::size_t)n_original, k::LPA_BLOCK, sc), k::LPA_BLOCK, 0, s>>>(
      comm, nid.data(), n_original);
  GRX_HIP_CHECK(hipGetLastError());
  tally.launches += 5;
  if (build) {
    // the entries keyed by (row, column) of the next level: sorted, then equal keys summed
    const std::size_t m = (std::size_t)lv.entries;
    hip::device_array_t<unsigned long long> key_in(m), key_sorted(m), key_out(m);
    hip::device_array_t<int32_t> w_in(m), w_sorted(m);
    hip::device_array_t<unsigned> count(1);
    next.own_aw = hip::device_array_t<int32_t>(m);  // at most as many distinct pairs as entries
    k::louvain_keys_kernel<W><<<grid_for(m, k::LPA_BLOCK, sc), k::LPA_BLOCK, 0, s>>>(
        lv.ap, lv.aj, lv.aw, nid.data(), n, lv.entries, key_in.data(), w_in.data());
    GRX_HIP_CHECK(hipGetLastError());
    int bits = 1;
    while ((1ll << bits) < next.n)
      ++bits;
    std::size_t sort_bytes = 0, reduce_bytes = 0;
    GRX_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, key_in.data(), key_sorted.data(), w_in.data(),
                                            w_sorted.data(), m, 0, 32 + bits, s));
    GRX_HIP_CHECK(rocprim::reduce_by_key(nullptr, reduce_bytes, key_sorted.data(), w_sorted.data(), m, key_out.data(),
                                         next.own_aw.data(), count.data(), rocprim::plus<int32_t>(),
                                         rocprim::equal_to<unsigned long long>(), s));
    hip::device_array_t<unsigned char> temp(std::max<std::size_t>(std::max(sort_bytes, reduce_bytes), 256));
    GRX_HIP_CHECK(rocprim::radix_sort_pairs(temp.data(), sort_bytes, key_in.data(), key_sorted.data(), w_in.data(),
                                            w_sorted.data(), m, 0, 32 + bits, s));
    GRX_HIP_CHECK(rocprim::reduce_by_key(temp.data(), reduce_bytes, key_sorted.data(), w_sorted.data(), m,
                                         key_out.data(), next.own_aw.data(), count.data(), rocprim::plus<int32_t>(),
                                         rocprim::equal_to<unsigned long long>(), s));
    unsigned distinct = 0;
    GRX_HIP_CHECK(hipMemcpyAsync(&distinct, count.data(), sizeof distinct, hipMemcpyDeviceToHost, s));
    GRX_HIP_CHECK(hipStreamSynchronize(s));
    error::throw_if_exception(distinct == 0 || distinct > m, "grx_louvain: the contraction lost its entries");
    next.entries = (int64_t)distinct;
    next.own_ap = hip::device_array_t<int32_t>((std::size_t)next.n + 1);
    next.own_aj = hip::device_array_t<int32_t>((std::size_t)distinct);
    k::louvain_unpack_kernel<<<grid_for(std::max<std::size_t>(distinct, (std::size_t)next.n + 1), k::LPA_BLOCK, sc),
                               k::LPA_BLOCK, 0, s>>>(key_out.data(), (int32_t)distinct, next.n, next.own_ap.data(),
                                                     next.own_aj.data());
    GRX_HIP_CHECK(hipGetLastError());
    GRX_HIP_CHECK(hipStreamSynchronize(s));  // the sorted keys are released behind it
    next.ap = next.own_ap.data();
    next.aj = next.own_aj.data();
    next.aw = next.own_aw.data();
    tally.launches += 4;
  }
  return next.n;
}

}  // namespace

extern "C" int grx_louvain(grx_context_t ctx, grx_graph_t g, int32_t* d_community, int64_t* h_communities,
                           double* h_modularity, int32_t* h_levels, const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_louvain: NULL argument");
  if (!d_community && !h_communities && !h_modularity && !h_levels)
    return invalid("grx_louvain: all four outputs are NULL");
  if (g->n_rows != g->n_cols)
    return invalid("grx_louvain: the graph is not square (n_rows != n_cols)");
  if (opt && opt->max_iterations < 0)
    return invalid("grx_louvain: max_iterations must not be negative");
  const bool timed = opt && opt->collect_kernel_time;
  const int32_t max_phases = opt ? opt->max_iterations : 0;
  return guarded([&] {
    const int32_t n = g->n_rows;
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (h_communities)
      *h_communities = 0;
    if (h_modularity)
      *h_modularity = 0.0;
    if (h_levels)
      *h_levels = 0;
    if (n == 0)  // the empty graph: nothing to write
      return (int)GRX_OK;
    if (int rc = require_symmetric(ctx, g, "grx_louvain", "modularity optimisation"))
      return rc;
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();

    const sweep_limits_t lim = sweep_limits("GRX_LOUVAIN");  // the test hooks and the LDS the device allows

    call_clock_t clock(s, timed);
    clock.start();

    tally_t tally;
    int32_t levels = 0, communities = n;
    {
      hip::device_array_t<int32_t> own_comm(d_community ? 0 : (std::size_t)n);
      int32_t* comm = d_community ? d_community : own_comm.data();
      hip::for_each_index_on((std::size_t)n, comm, s);

      auto lv = std::make_unique<level_t>();
      lv->n = n;
      lv->entries = g->nnz;
      lv->ap = g->d_ap;
      lv->aj = g->d_aj;
      for (;;) {
        hip::device_array_t<int32_t> label, tot;
        bool kept_any = false;
        int rc;
        if (levels == 0) {
          rc = run_phase<false>(ctx, g, *lv, lim, g->nnz, clock, tally, label, tot, kept_any);
        } else {
          grx_graph_s pattern;  // the level's pattern CSR behind a handle, for grx_color
          pattern.n_rows = pattern.n_cols = lv->n;
          pattern.nnz = lv->entries;
          pattern.d_ap = lv->ap;
          pattern.d_aj = lv->aj;
          pattern.symmetry = grx_graph_s::symmetric;  // contracted from a symmetric graph
          rc = run_phase<true>(ctx, &pattern, *lv, lim, g->nnz, clock, tally, label, tot, kept_any);
        }
        if (rc)
          return rc;
        ++levels;
        if (!kept_any)
          break;
        const bool last = levels == max_phases;
        auto next = std::make_unique<level_t>();
        communities = levels == 1
                          ? aggregate<false>(sc, *lv, label.data(), tot.data(), comm, n, !last, *next, tally)
                          : aggregate<true>(sc, *lv, label.data(), tot.data(), comm, n, !last, *next, tally);
        if (last)
          break;
        lv = std::move(next);
      }

      // the smallest original vertex names its community
      hip::device_array_t<unsigned> first((std::size_t)n);
      clock.begin_batch();
      GRX_HIP_CHECK(hipMemsetAsync(first.data(), 0xff, sizeof(unsigned) * (std::size_t)n, s));
      const unsigned grid = grid_for((std::size_t)n, k::LPA_BLOCK, sc);
      k::lpa_first_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(comm, n, first.data());
      k::louvain_name_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(comm, first.data(), n);
      GRX_HIP_CHECK(hipGetLastError());
      tally.launches += 2;
      clock.end_batch();
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();

    if (h_communities)
      *h_communities = (int64_t)communities;
    if (h_modularity)
      *h_modularity = modularity_of(tally.inside, tally.squares, g->nnz);
    if (h_levels)
      *h_levels = levels;
    if (stats) {
      const int32_t sweeps = (int32_t)tally.kept.size();
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->iterations = sweeps;
      stats->advance_launches = tally.launches;
      stats->vertices_reached = (int64_t)n - (int64_t)communities;
      stats->edges_traversed = g->nnz;
      stats->edges_expanded = tally.expanded;
      stats->levels_recorded = std::min(sweeps, 64);
      for (int32_t t = 0; t < stats->levels_recorded; ++t)
        stats->frontier_slots[t] = tally.kept[(std::size_t)t];
    }
    return (int)GRX_OK;
  });
}

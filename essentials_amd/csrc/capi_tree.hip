/** @file capi_tree.hip  grx_bfs_predecessors and grx_sssp_predecessors on one kernel family
 * (hip/kernels/tree_kernels.hxx): the shortest-path tree that finished labels imply, the count of
 * entries that contradict them, and hop counts by pointer doubling.  The labels are plain input: the
 * call runs on the caller's CSR as given, never on the hot-first copy, starts no symmetry verification
 * and leaves nothing on the handle.  The host waits once for label[source] before anything is
 * launched, once per batch of doubling rounds, and once for the call's figures at its end. */
#include "capi_batch.hxx"

#include <gunrock/hip/kernels/tree_kernels.hxx>

#include <cstdint>

using namespace essentials_amd;

namespace k = gunrock::hip::kernels;

namespace {

/// What a predecessors call may write; every pointer may be NULL, not all of them.
struct tree_outputs_t {
  int32_t* d_predecessors;
  int32_t* d_hops;
  int64_t* h_orphans;
  int64_t* h_violations;
};

template <typename label_t>
int tree_call(const char* call, grx_context_t ctx, grx_graph_t g, int32_t source, const label_t* d_labels,
              const tree_outputs_t& out, const grx_options* opt, grx_stats* stats) {
  constexpr bool weighted = k::tree_rule_t<label_t>::weighted;
  const std::string name(call);
  if (!ctx || !g)
    return invalid((name + ": NULL argument").c_str());
  if (g->n_rows != g->n_cols)
    return invalid((name + ": the graph is not square (n_rows != n_cols)").c_str());
  if (!out.d_predecessors && !out.d_hops && !out.h_orphans && !out.h_violations)
    return invalid((name + ": every output is NULL").c_str());
  const grx_options o = effective_options(opt);
  if (o.max_iterations != 0)
    return invalid((name + ": max_iterations must be 0 (the call is one pass, nothing to cut off)").c_str());
  const int32_t n = g->n_rows;
  const bool timed = o.collect_kernel_time != 0;
  return guarded([&] {
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (n == 0) {  // nothing is written, nothing is launched
      if (out.h_orphans)
        *out.h_orphans = 0;
      if (out.h_violations)
        *out.h_violations = 0;
      return (int)GRX_OK;
    }
    if (!d_labels)
      return invalid((name + ": the labels are NULL").c_str());
    if (source < 0 || source >= n)
      return invalid((name + ": source out of range").c_str());
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();
    label_t at_source;
    GRX_HIP_CHECK(hipMemcpyAsync(&at_source, d_labels + source, sizeof at_source, hipMemcpyDeviceToHost, s));
    GRX_HIP_CHECK(hipStreamSynchronize(s));
    if (at_source != (label_t)0)
      return invalid((name + ": label[source] is not 0: these are not the labels of a search from source").c_str());

    // pull over in-rows whenever somebody has already said what they are
    const bool own_rows_are_in_rows = g->symmetry == grx_graph_s::symmetric && (!weighted || g->weight_symmetric);
    const bool pull = env_flag("GRX_TREE_PULL", true) && (g->in_edges || own_rows_are_in_rows);
    const int32_t segment = (int32_t)env_or("GRX_TREE_SEGMENT", k::GROUP_SEGMENT, k::GROUP_SEGMENT_MIN, INT32_MAX);
    const std::size_t nv = (std::size_t)n;

    call_clock_t clock(s, timed);
    clock.start();
    int launches = 0, rounds = 0, moving_rounds = 0;
    unsigned long long h_counts[k::TREE_WORDS] = {};
    {
      hip::device_array_t<unsigned long long> counts(k::TREE_WORDS);
      hip::device_array_t<int32_t> own_pred;
      hip::device_array_t<int2> pairs;
      row_plan_t walk;
      int32_t* pred = out.d_predecessors;
      if (!pred) {
        own_pred = hip::device_array_t<int32_t>(nv);
        pred = own_pred.data();
      }
      clock.begin_batch();
      GRX_HIP_CHECK(hipMemsetAsync(counts.data(), 0, k::TREE_WORDS * sizeof(unsigned long long), s));
      launches += walk.build(pull ? in_rows(g) : out_rows(g), n, g->nnz, segment, sc);
      const unsigned per_vertex = grid_for(nv, k::GROUP_BLOCK, sc), per_row = walk.per_row(sc);
      if (pull) {
        k::tree_rows_kernel<label_t, false><<<per_row, k::GROUP_BLOCK, 0, s>>>(walk.rows, d_labels, n, segment, source,
                                                                              pred, counts.data());
        ++launches;
        if (walk.any_long) {
          k::tree_segment_kernel<label_t, false><<<walk.per_item(sc), k::GROUP_BLOCK, 0, s>>>(
              walk.rows, d_labels, walk.plan, segment, pred, counts.data());
          k::tree_fixup_kernel<label_t><<<walk.per_long_row(sc), k::GROUP_BLOCK, 0, s>>>(d_labels, walk.plan, source, pred,
                                                                                      counts.data());
          launches += 2;
        }
      } else {
        k::tree_fill_kernel<><<<per_vertex, k::GROUP_BLOCK, 0, s>>>(pred, n);
        k::tree_rows_kernel<label_t, true><<<per_row, k::GROUP_BLOCK, 0, s>>>(walk.rows, d_labels, n, segment, source,
                                                                             pred, counts.data());
        launches += 2;
        if (walk.any_long) {
          k::tree_segment_kernel<label_t, true><<<walk.per_item(sc), k::GROUP_BLOCK, 0, s>>>(
              walk.rows, d_labels, walk.plan, segment, pred, counts.data());
          ++launches;
        }
        k::tree_finalise_kernel<label_t><<<per_vertex, k::GROUP_BLOCK, 0, s>>>(d_labels, n, source, pred, counts.data());
        ++launches;
      }
      if (out.d_hops) {
        pairs = hip::device_array_t<int2>(2 * nv);
        int2* pair[2] = {pairs.data(), pairs.data() + nv};
        k::tree_hops_begin_kernel<><<<per_vertex, k::GROUP_BLOCK, 0, s>>>(pred, n, pair[0]);
        ++launches;
        unsigned long long* changed = counts.data() + k::TREE_CHANGED;
        for (bool settled = false; !settled;) {
          // a chain of fewer than 2^31 steps is at its end after 31 rounds, and the 32nd changes nothing
          error::throw_if_exception(rounds >= 32, name + ": the chains are not at their ends after 32 rounds");
          for (int j = 0; j < k::TREE_ROUNDS_AHEAD; ++j)  // a round past the last changing one copies
            k::tree_hops_round_kernel<><<<per_vertex, k::GROUP_BLOCK, 0, s>>>(pair[(rounds + j) & 1],
                                                                           pair[~(rounds + j) & 1], n, changed + j);
          launches += k::TREE_ROUNDS_AHEAD + 1;
          unsigned long long* m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
            k::tree_hops_publish_kernel<><<<1, 1, 0, s>>>(changed, mirror, slot, seq);
          });
          for (int j = 0; j < k::TREE_ROUNDS_AHEAD && !settled; ++j) {
            settled = m[k::TM_CHANGED + j] == 0;
            moving_rounds += settled ? 0 : 1;
          }
          rounds += k::TREE_ROUNDS_AHEAD;
          clock.begin_batch();
        }
        k::tree_hops_end_kernel<><<<per_vertex, k::GROUP_BLOCK, 0, s>>>(pair[rounds & 1], n, source, out.d_hops);
        ++launches;
      }
      GRX_HIP_CHECK(hipGetLastError());
      clock.end_batch();
      GRX_HIP_CHECK(hipMemcpyAsync(h_counts, counts.data(), sizeof h_counts, hipMemcpyDeviceToHost, s));
      GRX_HIP_CHECK(hipStreamSynchronize(s));
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();

    if (out.h_orphans)
      *out.h_orphans = (int64_t)h_counts[k::TREE_N_ORPHANS];
    if (out.h_violations)
      *out.h_violations = (int64_t)h_counts[k::TREE_N_VIOLATIONS];
    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->advance_launches = launches;
      stats->vertices_reached = (int64_t)h_counts[k::TREE_N_REACHED];
      stats->edges_traversed = stats->edges_expanded = g->nnz;
      stats->pull_iterations = pull ? 1 : 0;
      // the rounds that moved a pair: ceil(log2(longest chain))
      stats->iterations = moving_rounds;
    }
    return (int)GRX_OK;
  });
}

}  // namespace

extern "C" int grx_bfs_predecessors(grx_context_t ctx, grx_graph_t g, int32_t source, const int32_t* d_depths,
                                    int32_t* d_predecessors, int64_t* h_orphans, int64_t* h_violations,
                                    const grx_options* opt, grx_stats* stats) {
  return tree_call<int32_t>("grx_bfs_predecessors", ctx, g, source, d_depths,
                            tree_outputs_t{d_predecessors, nullptr, h_orphans, h_violations}, opt, stats);
}

extern "C" int grx_sssp_predecessors(grx_context_t ctx, grx_graph_t g, int32_t source, const float* d_distances,
                                     int32_t* d_predecessors, int32_t* d_hops, int64_t* h_orphans,
                                     int64_t* h_violations, const grx_options* opt, grx_stats* stats) {
  return tree_call<float>("grx_sssp_predecessors", ctx, g, source, d_distances,
                          tree_outputs_t{d_predecessors, d_hops, h_orphans, h_violations}, opt, stats);
}

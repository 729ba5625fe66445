/** @file capi_softmax.hip  grx_edge_softmax and grx_edge_softmax_backward: per-entry scores normalised over
 * the entries of a row, or of a column (hip/kernels/softmax_kernels.hxx), and the derivative of that.  The
 * groups are the rows of the CSR's offsets or of the attached in-rows', long ones cut into items by the plan
 * of the lane-group sweep (capi_batch.hxx: row_plan_t); by column the kernels reach an entry through the
 * in-edges' entry ids (graph::transposed_t::edge_ids) where they walk, so nothing is gathered or scattered
 * in a pass of its own. */
#include "capi_dense.hxx"

#include <gunrock/graph/transpose.hxx>
#include <gunrock/hip/kernels/softmax_kernels.hxx>

#include <cstdint>

using namespace essentials_amd;

namespace k = gunrock::hip::kernels;

namespace {

/// The entries one lane group takes of a long group (a test hook, read per call).
int32_t segment_entries() {
  return (int32_t)env_or("GRX_SOFTMAX_SEGMENT", k::GROUP_SEGMENT, k::GROUP_SEGMENT_MIN, INT32_MAX);
}

/// The groups of a call, the list of its long ones and, per item the list has room for, a partial sum
/// and -- at a long group's first item -- its total and the key of its maximum.
struct softmax_rows_t : row_plan_t {
  hip::device_array_t<float> partial, total;
  hip::device_array_t<unsigned> max_keys;
  k::softmax_groups_t groups{};

  /// Enqueue the plan; returns the launches.
  int build(const grx_graph_s* g, bool by_column, bool forward, int32_t seg, gcuda::standard_context_t& sc) {
    const int launches = row_plan_t::build(by_column ? in_rows(g) : out_rows(g), g->n_rows, g->nnz, seg, sc);
    groups = k::softmax_groups_t{rows.ap, by_column ? g->in_edges->edge_ids.data() : nullptr, n, segment};
    if (any_long) {
      partial = hip::device_array_t<float>((std::size_t)plan.most_items);
      total = hip::device_array_t<float>((std::size_t)plan.most_items);
      if (forward) {
        max_keys = hip::device_array_t<unsigned>((std::size_t)plan.most_items);
        GRX_HIP_CHECK(hipMemsetAsync(max_keys.data(), 0, (std::size_t)plan.most_items * sizeof(unsigned), sc.stream()));
      }
    }
    return launches;
  }

  /// Enqueue out = softmax(s) per group; returns the launches.
  template <bool INDIRECT>
  int forward(const float* s, float* out, gcuda::standard_context_t& sc) const {
    const hipStream_t q = sc.stream();
    k::softmax_rows_kernel<INDIRECT><<<per_row(sc), k::GROUP_BLOCK, 0, q>>>(groups, s, out);
    if (!any_long)
      return 1;
    k::softmax_item_max_kernel<INDIRECT><<<per_item(sc), k::GROUP_BLOCK, 0, q>>>(groups, plan, s, max_keys.data());
    k::softmax_item_sum_kernel<INDIRECT><<<per_item(sc), k::GROUP_BLOCK, 0, q>>>(groups, plan, s, max_keys.data(),
                                                                                partial.data());
    k::softmax_combine_kernel<><<<per_long_row(sc), k::GROUP_BLOCK, 0, q>>>(groups, plan, partial.data(), total.data());
    k::softmax_item_write_kernel<INDIRECT><<<per_item(sc), k::GROUP_BLOCK, 0, q>>>(groups, plan, s, max_keys.data(),
                                                                                  total.data(), out);
    return 5;
  }

  /// Enqueue out = a * (t - <a, t> per group); returns the launches.
  template <bool INDIRECT>
  int backward(const float* a, const float* t, float* out, gcuda::standard_context_t& sc) const {
    const hipStream_t q = sc.stream();
    k::softmax_backward_rows_kernel<INDIRECT><<<per_row(sc), k::GROUP_BLOCK, 0, q>>>(groups, a, t, out);
    if (!any_long)
      return 1;
    k::softmax_backward_item_sum_kernel<INDIRECT><<<per_item(sc), k::GROUP_BLOCK, 0, q>>>(groups, plan, a, t,
                                                                                         partial.data());
    k::softmax_combine_kernel<><<<per_long_row(sc), k::GROUP_BLOCK, 0, q>>>(groups, plan, partial.data(), total.data());
    k::softmax_backward_item_write_kernel<INDIRECT><<<per_item(sc), k::GROUP_BLOCK, 0, q>>>(groups, plan, a, t,
                                                                                           total.data(), out);
    return 4;
  }
};

/// grx_edge_softmax (`d_second` NULL: d_first holds the scores) and grx_edge_softmax_backward (d_first
/// the probabilities, d_second the gradient) are one call.
int softmax_call(const char* call, bool forward, grx_context_t ctx, grx_graph_t g, int32_t by_column,
                 const float* d_first, const float* d_second, float* d_out, const grx_options* opt, grx_stats* stats) {
  const std::string name(call);
  const auto refuse = [&](const char* why) { return invalid((name + ": " + why).c_str()); };
  if (!ctx || !g)
    return refuse("NULL argument");
  const std::size_t nnz = (std::size_t)g->nnz;
  const byte_range_t range_first(d_first, nnz, 1, 1), range_second(forward ? nullptr : d_second, forward ? 0 : nnz, 1, 1);
  const byte_range_t range_out(d_out, nnz, 1, 1);
  if (nnz && (!d_first || !d_out || (!forward && !d_second)))
    return refuse(forward ? "d_scores or d_out is NULL" : "d_probabilities, d_grad or d_out is NULL");
  if (range_out.meets(range_first) || range_out.meets(range_second))
    return refuse(forward ? "the byte range of d_out overlaps that of d_scores"
                          : "the byte range of d_out overlaps that of d_probabilities or d_grad");
  if (by_column && g->n_rows != g->n_cols)
    return unsupported((name + ": by column on a graph that is not square (n_rows != n_cols)").c_str());
  if (by_column && !g->in_edges)  // a column's entries are found through the entry ids alone
    return unsupported((name + ": by column needs the in-edges and their entry ids, on a symmetric CSR too: call "
                               "grx_graph_build_in_edges first")
                           .c_str());
  const bool timed = effective_options(opt).collect_kernel_time != 0;
  return guarded([&] {
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (g->nnz == 0)  // nothing to write: nothing is launched
      return (int)GRX_OK;
    auto& sc = ctx->single();
    call_clock_t clock(sc.stream(), timed);
    clock.start();
    int launches = 0;
    {
      softmax_rows_t p;
      clock.begin_batch();
      launches += p.build(g, by_column != 0, forward, segment_entries(), sc);
      if (forward)
        launches += by_column ? p.forward<true>(d_first, d_out, sc) : p.forward<false>(d_first, d_out, sc);
      else
        launches += by_column ? p.backward<true>(d_first, d_second, d_out, sc)
                              : p.backward<false>(d_first, d_second, d_out, sc);
      GRX_HIP_CHECK(hipGetLastError());
      clock.end_batch();
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();
    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->advance_launches = launches;
      stats->iterations = 1;
      stats->edges_traversed = stats->edges_expanded = g->nnz;
    }
    return (int)GRX_OK;
  });
}

}  // namespace

extern "C" int grx_edge_softmax(grx_context_t ctx, grx_graph_t g, int32_t by_column, const float* d_scores,
                                float* d_out, const grx_options* opt, grx_stats* stats) {
  return softmax_call("grx_edge_softmax", true, ctx, g, by_column, d_scores, nullptr, d_out, opt, stats);
}

extern "C" int grx_edge_softmax_backward(grx_context_t ctx, grx_graph_t g, int32_t by_column,
                                         const float* d_probabilities, const float* d_grad, float* d_out,
                                         const grx_options* opt, grx_stats* stats) {
  return softmax_call("grx_edge_softmax_backward", false, ctx, g, by_column, d_probabilities, d_grad, d_out, opt,
                      stats);
}

/** @file capi_spmm.hip  grx_spmm: the sparse-dense product Y = A X (hip/kernels/spmm_kernels.hxx), features on
 * the lanes and a row's entries in row order, long rows cut into segments by the plan of the lane-group
 * sweep (capi_batch.hxx: row_plan_t) and their partial sums added in segment order.  Which lane-group
 * width and which access width serve a call is decided here, once per call.  grx_spmm_values is the same
 * call with the caller's per-entry values where the sweep reads its weights: as they are forward, gathered
 * into in-entry order through the in-edges' entry ids (graph::transposed_t::edge_ids) transposed. */
#include "capi_dense.hxx"

#include <gunrock/graph/transpose.hxx>
#include <gunrock/hip/kernels/spmm_kernels.hxx>

#include <cstdint>

using namespace essentials_amd;

namespace k = gunrock::hip::kernels;

namespace {

/// The entries one partial sum takes (a test hook, read per call).
int32_t segment_entries() {
  return (int32_t)env_or("GRX_SPMM_SEGMENT", k::GROUP_SEGMENT, k::GROUP_SEGMENT_MIN, INT32_MAX);
}

/// The rows of a product, the list of its long ones and the room for their partial sums.
struct dense_rows_t : row_plan_t {
  hip::device_array_t<float> partial;

  /// Enqueue the plan; returns the launches.
  int build(const k::csr_rows_t& r, int32_t n_rows, int64_t nnz, int32_t seg, int32_t F,
            gcuda::standard_context_t& sc) {
    const int launches = row_plan_t::build(r, n_rows, nnz, seg, sc);
    if (any_long)
      partial = hip::device_array_t<float>((std::size_t)plan.most_items * (std::size_t)F);
    return launches;
  }

  template <int L, bool VEC>
  int product(const k::spmm_operands_t& m, gcuda::standard_context_t& sc) const {
    const hipStream_t s = sc.stream();
    constexpr int PER_BLOCK = k::GROUP_BLOCK / L;
    const unsigned tiles = (unsigned)((m.F + k::SPMM_TILE - 1) / k::SPMM_TILE);
    k::spmm_gather_kernel<L, VEC><<<dim3(odd_grid_for(n, PER_BLOCK, sc), tiles), k::GROUP_BLOCK, 0, s>>>(
        rows, n, segment, m);
    if (!any_long)
      return 1;
    k::spmm_segment_kernel<L, VEC><<<dim3(grid_for(plan.most_items, PER_BLOCK, sc), tiles), k::GROUP_BLOCK, 0, s>>>(
        rows, plan, segment, m, partial.data());
    k::spmm_combine_kernel<><<<grid_for((std::size_t)plan.most_rows * (std::size_t)m.F, k::GROUP_BLOCK, sc),
                               k::GROUP_BLOCK, 0, s>>>(rows, plan, segment, m, partial.data());
    return 3;
  }

  template <int L>
  int product(const k::spmm_operands_t& m, bool vec_x, gcuda::standard_context_t& sc) const {
    return vec_x ? product<L, true>(m, sc) : product<L, false>(m, sc);
  }

  /// Enqueue Y = rows * X; returns the launches.
  int product(const k::spmm_operands_t& m, gcuda::standard_context_t& sc) const {
    const bool vec_x = sixteen(m.x, m.ldx);
    switch (lanes_for(m.F)) {
      case 1: return product<1>(m, vec_x, sc);
      case 2: return product<2>(m, vec_x, sc);
      case 4: return product<4>(m, vec_x, sc);
      case 8: return product<8>(m, vec_x, sc);
      case 16: return product<16>(m, vec_x, sc);
      case 32: return product<32>(m, vec_x, sc);
      default: return product<64>(m, vec_x, sc);
    }
  }
};

/// grx_spmm (`values` false: the handle's values) and grx_spmm_values (the caller's d_values, in the
/// CSR's entry order) are one call.
int product_call(const char* call, grx_context_t ctx, grx_graph_t g, bool values, const float* d_values,
                 int32_t transpose, int32_t n_features, const float* d_x, int64_t ldx, float* d_y, int64_t ldy,
                 const grx_options* opt, grx_stats* stats) {
  const std::string name(call);
  const auto refuse = [&](const char* why) { return invalid((name + ": " + why).c_str()); };
  if (!ctx || !g)
    return refuse("NULL argument");
  const int32_t F = n_features;
  if (F < 0)
    return refuse("n_features < 0");
  if (ldx < F || ldy < F)
    return refuse("ldx or ldy is below n_features");
  const std::size_t rows_x = (std::size_t)(transpose ? g->n_rows : g->n_cols);
  const std::size_t rows_y = (std::size_t)(transpose ? g->n_cols : g->n_rows);
  const byte_range_t range_x(d_x, rows_x, ldx, F), range_y(d_y, rows_y, ldy, F);
  if ((!d_x && !range_x.empty()) || (!d_y && !range_y.empty()))
    return refuse("d_x or d_y is NULL");
  if (range_x.meets(range_y))
    return refuse("the byte ranges of d_x and d_y overlap");
  if (values) {
    if (!d_values && g->nnz > 0)
      return refuse("d_values is NULL");
    if (byte_range_t(d_values, (std::size_t)g->nnz, 1, 1).meets(range_y))
      return refuse("the byte ranges of d_values and d_y overlap");
  }
  if (transpose && g->n_rows != g->n_cols)
    return unsupported((name + ": the transposed product of a graph that is not square (n_rows != n_cols)").c_str());
  if (values && transpose && !g->in_edges)  // a mirror entry's value sits elsewhere in d_values
    return unsupported((name + ": the transposed product with the caller's values needs the in-edges and their "
                               "entry ids, on a symmetric CSR too: call grx_graph_build_in_edges first")
                           .c_str());
  const bool timed = effective_options(opt).collect_kernel_time != 0;
  return guarded([&] {
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (F == 0 || rows_y == 0)  // nothing to write: nothing is launched
      return (int)GRX_OK;
    if (transpose && !g->in_edges)
      if (int rc = ensure_can_pull(ctx, g)) {  // the handle's rows must be its in-rows too
        last_error() = name + ": " + last_error();
        return rc;
      }
    auto& sc = ctx->single();
    call_clock_t clock(sc.stream(), timed);
    clock.start();
    int launches = 0;
    {
      dense_rows_t p;
      hip::device_array_t<float> in_values;  // d_values in the order of the in-entries
      const k::spmm_operands_t m{d_x, ldx, d_y, ldy, F, sixteen(d_y, ldy) ? 1 : 0};
      k::csr_rows_t rows = transpose ? in_rows(g) : out_rows(g);
      clock.begin_batch();
      if (values && transpose && g->nnz > 0) {
        in_values = hip::device_array_t<float>((std::size_t)g->nnz);
        gunrock::graph::detail::gather_kernel<<<grid_for((std::size_t)g->nnz, 256, sc), 256, 0, sc.stream()>>>(
            d_values, g->in_edges->edge_ids.data(), (long long)g->nnz, in_values.data());
        rows.ax = in_values.data();
        ++launches;
      } else if (values) {
        rows.ax = d_values;
      }
      launches += p.build(rows, (int32_t)rows_y, g->nnz, segment_entries(), F, sc);
      launches += p.product(m, sc);
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

extern "C" int grx_spmm(grx_context_t ctx, grx_graph_t g, int32_t transpose, int32_t n_features, const float* d_x,
                        int64_t ldx, float* d_y, int64_t ldy, const grx_options* opt, grx_stats* stats) {
  return product_call("grx_spmm", ctx, g, false, nullptr, transpose, n_features, d_x, ldx, d_y, ldy, opt, stats);
}

extern "C" int grx_spmm_values(grx_context_t ctx, grx_graph_t g, const float* d_values, int32_t transpose,
                               int32_t n_features, const float* d_x, int64_t ldx, float* d_y, int64_t ldy,
                               const grx_options* opt, grx_stats* stats) {
  return product_call("grx_spmm_values", ctx, g, true, d_values, transpose, n_features, d_x, ldx, d_y, ldy, opt,
                      stats);
}

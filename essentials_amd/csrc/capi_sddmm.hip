/** @file capi_sddmm.hip  grx_sddmm: the per-entry dot products out[e] = <U[row(e)], V[col(e)]>
 * (hip/kernels/sddmm_kernels.hxx), features on the lanes and a row's entries in time, long rows handed out
 * as items by the plan of the lane-group sweep (capi_batch.hxx: row_plan_t).  Which lane-group width and
 * which access width serve a call is decided here, once per call. */
#include "capi_dense.hxx"

#include <gunrock/hip/kernels/sddmm_kernels.hxx>

#include <cstdint>

using namespace essentials_amd;

namespace k = gunrock::hip::kernels;

namespace {

/// The entries one lane group takes of a long row (a test hook, read per call).
int32_t segment_entries() {
  return (int32_t)env_or("GRX_SDDMM_SEGMENT", k::GROUP_SEGMENT, k::GROUP_SEGMENT_MIN, INT32_MAX);
}

constexpr int WAVE = k::SPMM_TILE / k::SPMM_VEC;  // the lanes a feature tile takes

/// The rows of a call and the list of its long ones.
struct edge_rows_t : row_plan_t {
  template <int L, bool VEC, bool TILED>
  int products(const k::sddmm_operands_t& m, gcuda::standard_context_t& sc) const {
    const hipStream_t s = sc.stream();
    constexpr int PER_BLOCK = k::GROUP_BLOCK / L;
    k::sddmm_rows_kernel<L, VEC, TILED><<<odd_grid_for(n, PER_BLOCK, sc), k::GROUP_BLOCK, 0, s>>>(rows, n, segment, m);
    if (!any_long)
      return 1;
    k::sddmm_items_kernel<L, VEC, TILED><<<grid_for(plan.most_items, PER_BLOCK, sc), k::GROUP_BLOCK, 0, s>>>(
        rows, plan, segment, m);
    return 2;
  }

  template <int L>
  int products(const k::sddmm_operands_t& m, bool vec, gcuda::standard_context_t& sc) const {
    return vec ? products<L, true, false>(m, sc) : products<L, false, false>(m, sc);
  }

  /// Enqueue out[e] for every entry; returns the launches.
  int products(const k::sddmm_operands_t& m, gcuda::standard_context_t& sc) const {
    const bool vec = sixteen(m.u, m.ldu) && sixteen(m.v, m.ldv);
    if (m.F > k::SPMM_TILE)
      return vec ? products<WAVE, true, true>(m, sc) : products<WAVE, false, true>(m, sc);
    switch (lanes_for(m.F)) {
      case 1: return products<1>(m, vec, sc);
      case 2: return products<2>(m, vec, sc);
      case 4: return products<4>(m, vec, sc);
      case 8: return products<8>(m, vec, sc);
      case 16: return products<16>(m, vec, sc);
      case 32: return products<32>(m, vec, sc);
      default: return products<64>(m, vec, sc);
    }
  }
};

}  // namespace

extern "C" int grx_sddmm(grx_context_t ctx, grx_graph_t g, int32_t n_features, const float* d_u, int64_t ldu,
                         const float* d_v, int64_t ldv, float* d_out, const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_sddmm: NULL argument");
  const int32_t F = n_features;
  if (F < 0)
    return invalid("grx_sddmm: n_features < 0");
  if (ldu < F || ldv < F)
    return invalid("grx_sddmm: ldu or ldv is below n_features");
  const byte_range_t range_u(d_u, (std::size_t)g->n_rows, ldu, F), range_v(d_v, (std::size_t)g->n_cols, ldv, F);
  const byte_range_t range_out(d_out, (std::size_t)g->nnz, 1, 1);
  if ((!d_u && !range_u.empty()) || (!d_v && !range_v.empty()) || (!d_out && !range_out.empty()))
    return invalid("grx_sddmm: d_u, d_v or d_out is NULL");
  if (range_out.meets(range_u) || range_out.meets(range_v))
    return invalid("grx_sddmm: the byte range of d_out overlaps that of d_u or d_v");
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
      edge_rows_t p;
      const k::sddmm_operands_t m{d_u, ldu, d_v, ldv, d_out, F};
      clock.begin_batch();
      if (F == 0) {  // an empty sum
        GRX_HIP_CHECK(hipMemsetAsync(d_out, 0, (std::size_t)g->nnz * sizeof(float), sc.stream()));
      } else {
        launches += p.build(out_rows(g), g->n_rows, g->nnz, segment_entries(), sc);
        launches += p.products(m, sc);
        GRX_HIP_CHECK(hipGetLastError());
      }
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

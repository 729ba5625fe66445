/** @file capi_spmv.hip  grx_spmv and grx_hits on one kernel family (hip/kernels/spmv_kernels.hxx): row sums
 * in a fixed order by 16-lane groups, long rows cut into segments once per call.  grx_hits is not the
 * reference's hits.hxx (two float-atomic scatters, an L2 norm, a bit-equality stop): two pull products
 * per iteration, normalised by the largest magnitude, whose scale is applied where the next product
 * gathers the value.  Nothing here waits for the host except the per-iteration hand-off of a run that
 * stops by tol and the read of the call's figures at its end. */
#include "capi_batch.hxx"

#include <gunrock/hip/kernels/spmv_kernels.hxx>

#include <cmath>
#include <cstdint>

using namespace essentials_amd;

namespace k = gunrock::hip::kernels;

namespace {

/// The entries one lane group sums (a test hook, read per call).
int32_t segment_entries() {
  return (int32_t)env_or("GRX_SPMV_SEGMENT", k::GROUP_SEGMENT, k::GROUP_SEGMENT_MIN, INT32_MAX);
}

/// The rows of a product, the list of its long ones and the room for their partial sums.
struct product_rows_t : row_plan_t {
  hip::device_array_t<float> partial;

  /// Enqueue the plan; returns the launches.
  int build(const k::csr_rows_t& r, int32_t n_rows, int64_t nnz, int32_t seg, gcuda::standard_context_t& sc) {
    const int launches = row_plan_t::build(r, n_rows, nnz, seg, sc);
    if (any_long)
      partial = hip::device_array_t<float>((std::size_t)plan.most_items);
    return launches;
  }

  /// Enqueue y = rows * (x scaled by the word at scale_bits); returns the launches.
  template <bool SCALED, bool TRACK>
  int product(const float* x, const unsigned* scale_bits, float* y, unsigned* max_bits,
              gcuda::standard_context_t& sc) const {
    const hipStream_t s = sc.stream();
    k::spmv_gather_kernel<SCALED, TRACK><<<per_row(sc), k::GROUP_BLOCK, 0, s>>>(rows, x, scale_bits, n, segment, y,
                                                                              max_bits);
    if (!any_long)
      return 1;
    k::spmv_segment_kernel<SCALED><<<per_item(sc), k::GROUP_BLOCK, 0, s>>>(rows, x, scale_bits, plan, segment,
                                                                         partial.data());
    k::spmv_combine_kernel<TRACK><<<per_long_row(sc), k::GROUP_BLOCK, 0, s>>>(rows, plan, segment, partial.data(), y,
                                                                            max_bits);
    return 3;
  }
};

bool overlap(const float* a, std::size_t na, const float* b, std::size_t nb) {
  const std::uintptr_t a0 = (std::uintptr_t)a, b0 = (std::uintptr_t)b;
  return na && nb && a0 < b0 + nb * sizeof(float) && b0 < a0 + na * sizeof(float);
}

}  // namespace

extern "C" int grx_spmv(grx_context_t ctx, grx_graph_t g, int32_t transpose, const float* d_x, float* d_y,
                        const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_spmv: NULL argument");
  if (transpose && g->n_rows != g->n_cols)
    return unsupported("grx_spmv: the transposed product of a graph that is not square (n_rows != n_cols)");
  const std::size_t len_x = (std::size_t)(transpose ? g->n_rows : g->n_cols);
  const std::size_t len_y = (std::size_t)(transpose ? g->n_cols : g->n_rows);
  if ((!d_x && len_x) || (!d_y && len_y))
    return invalid("grx_spmv: d_x or d_y is NULL");
  if (overlap(d_x, len_x, d_y, len_y))
    return invalid("grx_spmv: d_x and d_y overlap");
  const bool timed = effective_options(opt).collect_kernel_time != 0;
  return guarded([&] {
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (len_y == 0)  // nothing to write: nothing is launched
      return (int)GRX_OK;
    if (transpose && !g->in_edges)
      if (int rc = ensure_can_pull(ctx, g)) {  // the handle's rows must be its in-rows too
        last_error() = "grx_spmv: " + last_error();
        return rc;
      }
    auto& sc = ctx->single();
    call_clock_t clock(sc.stream(), timed);
    clock.start();
    int launches = 0;
    {
      product_rows_t p;
      clock.begin_batch();
      launches += p.build(transpose ? in_rows(g) : out_rows(g), (int32_t)len_y, g->nnz, segment_entries(), sc);
      launches += p.product<false, false>(d_x, nullptr, d_y, nullptr, sc);
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

extern "C" int grx_hits(grx_context_t ctx, grx_graph_t g, float tol, float* d_hub, float* d_authority,
                        int32_t* h_iterations, float* h_residual, const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_hits: NULL argument");
  if (g->n_rows != g->n_cols)
    return invalid("grx_hits: the graph is not square (n_rows != n_cols)");
  const int32_t n = g->n_rows;
  if (!d_hub && !d_authority && n > 0)
    return invalid("grx_hits: d_hub and d_authority are both NULL");
  if (std::isnan(tol))
    return invalid("grx_hits: tol is NaN");
  const grx_options o = effective_options(opt);
  if (o.max_iterations < 0)
    return invalid("grx_hits: max_iterations < 0");
  if (tol <= 0.0f && o.max_iterations == 0)
    return invalid("grx_hits: tol <= 0 (never by tol) needs max_iterations > 0");
  const bool timed = o.collect_kernel_time != 0, by_tol = tol > 0.0f;
  return guarded([&] {
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (n == 0)  // nothing is written, nothing is launched
      return (int)GRX_OK;
    if (int rc = ensure_can_pull(ctx, g)) {  // the authority product runs over in-entries
      last_error() = "grx_hits: " + last_error();
      return rc;
    }
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();
    const int32_t segment = segment_entries();
    const std::size_t nv = (std::size_t)n;

    call_clock_t clock(s, timed);
    clock.start();
    long long launches = 0;
    k::hits_ctl_t h_ctl{};
    {
      // per vertex the unnormalised products: y and the two z that take turns
      hip::device_array_t<float> state(3 * nv);
      hip::device_array_t<k::hits_ctl_t> control(1);
      float* y = state.data();
      float* z[2] = {state.data() + nv, state.data() + 2 * nv};
      k::hits_ctl_t* ctl = control.data();

      // once per call: the long rows, and the long in-rows when those are other arrays
      product_rows_t out, in_own;
      clock.begin_batch();
      launches += out.build(out_rows(g), n, g->nnz, segment, sc);
      if (g->in_edges)
        launches += in_own.build(in_rows(g), n, g->nnz, segment, sc);
      const product_rows_t& in = g->in_edges ? in_own : out;
      k::hits_begin_kernel<><<<grid_for(nv, k::GROUP_BLOCK, sc), k::GROUP_BLOCK, 0, s>>>(z[0], n, ctl);
      ++launches;

      int32_t t = 0;
      for (;;) {
        ++t;
        // a run that contracts stops long before this; NaN weights never do
        error::throw_if_exception(t > (1 << 20), "grx_hits: not below tol after 2^20 iterations");
        const int now = t & 1, old = now ^ 1;
        const bool last = o.max_iterations && t >= o.max_iterations;
        launches += in.product<true, true>(z[old], &ctl->h_max[old], y, &ctl->a_max, sc);
        launches += out.product<true, true>(y, &ctl->a_max, z[now], &ctl->h_max[now], sc);
        if (by_tol || last) {  // otherwise nobody reads this iteration's residual
          k::hits_residual_kernel<><<<grid_for(nv, k::GROUP_BLOCK, sc), k::GROUP_BLOCK, 0, s>>>(z[0], z[1], now, n, ctl);
          ++launches;
        }
        ++launches;
        if (!by_tol) {
          k::hits_step_kernel<><<<1, 1, 0, s>>>(ctl, t, last ? 1 : 0, nullptr, 0, 0ull);
          if (last)
            break;
          continue;
        }
        unsigned long long* m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
          k::hits_step_kernel<><<<1, 1, 0, s>>>(ctl, t, 1, mirror, slot, seq);
        });
        const unsigned bits = (unsigned)m[k::HM_DIFF];
        float diff;
        std::memcpy(&diff, &bits, sizeof diff);
        clock.begin_batch();
        if (diff < tol || last)
          break;
      }
      k::hits_deliver_kernel<><<<grid_for(nv, k::GROUP_BLOCK, sc), k::GROUP_BLOCK, 0, s>>>(z[t & 1], y, t & 1, n, d_hub,
                                                                                        d_authority, ctl);
      GRX_HIP_CHECK(hipGetLastError());
      clock.end_batch();
      ++launches;
      GRX_HIP_CHECK(hipMemcpyAsync(&h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost, s));
      GRX_HIP_CHECK(hipStreamSynchronize(s));
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();

    if (h_iterations)
      *h_iterations = h_ctl.iterations;
    if (h_residual)
      *h_residual = h_ctl.residual;
    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->iterations = h_ctl.iterations;
      stats->advance_launches = (int32_t)std::min<long long>(launches, INT32_MAX);
      stats->vertices_reached = (int64_t)h_ctl.reached;
      stats->edges_traversed = stats->edges_expanded = 2 * (int64_t)g->nnz * (int64_t)h_ctl.iterations;
    }
    return (int)GRX_OK;
  });
}

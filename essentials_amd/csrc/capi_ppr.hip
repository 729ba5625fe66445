/** @file capi_ppr.hip  grx_ppr: personalized PageRank from many seeds, 64 columns to a wavefront
 * (hip/kernels/ppr_kernels.hxx).  Not the reference's ppr.hxx (an approximate forward push with float
 * atomics): a power iteration over in-entries whose every sum has a fixed order.  Once per call the
 * scale vector and the two lists (dangling vertices, long in-rows); per batch a seed kernel, then per
 * iteration gather, segment + combine, dangling and the publish kernel -- one hand-off per iteration --
 * and the transposing delivery. */
#include "capi_batch.hxx"

#include <gunrock/hip/kernels/ppr_kernels.hxx>

#include <cmath>

using namespace essentials_amd;

namespace k = gunrock::hip::kernels;

namespace {

/// out[0, *count) = the i in [0, n) with flags[i] != 0, ascending (rocprim::select keeps the order).
void list_flagged(const unsigned char* flags, std::size_t n, int32_t* out, int32_t* count, hipStream_t s) {
  std::size_t bytes = 0;
  rocprim::counting_iterator<int32_t> ids(0);
  GRX_HIP_CHECK(rocprim::select(nullptr, bytes, ids, flags, out, count, n, s));
  hip::buffer_t<unsigned char> temp(bytes < 256 ? 256 : bytes);  // never a null temp: that is a size query
  GRX_HIP_CHECK(rocprim::select(temp.data(), bytes, ids, flags, out, count, n, s));
}

/// f(std::integral_constant<int, L>) for the batch's width class.
template <typename F>
void with_width(int L, F&& f) {
  if (L == 16)
    f(std::integral_constant<int, 16>());
  else if (L == 32)
    f(std::integral_constant<int, 32>());
  else
    f(std::integral_constant<int, 64>());
}

}  // namespace

extern "C" int grx_ppr(grx_context_t ctx, grx_graph_t g, const int32_t* h_seeds, int32_t n_seeds, float alpha,
                       float tol, float* d_p, int32_t* h_iterations, float* h_residual, const grx_options* opt,
                       grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_ppr: NULL argument");
  if (n_seeds < 0)
    return invalid("grx_ppr: n_seeds < 0");
  if (!h_seeds && n_seeds != 0)
    return invalid("grx_ppr: h_seeds is NULL (every vertex) but n_seeds != 0");
  for (int32_t i = 0; i < n_seeds; ++i)
    if (h_seeds[i] < 0 || h_seeds[i] >= g->n_rows)
      return invalid("grx_ppr: seed out of range");
  if (g->n_rows != g->n_cols)
    return invalid("grx_ppr: the graph is not square (n_rows != n_cols)");
  if (!(alpha >= 0.0f && alpha < 1.0f))
    return invalid("grx_ppr: alpha must be in [0, 1)");
  if (std::isnan(tol))
    return invalid("grx_ppr: tol is NaN");
  const grx_options o = effective_options(opt);
  if (o.max_iterations < 0)
    return invalid("grx_ppr: max_iterations < 0");
  if (tol <= 0.0f && o.max_iterations == 0)
    return invalid("grx_ppr: tol <= 0 (never by tol) needs max_iterations > 0");
  const int32_t n = g->n_rows;
  const int64_t count = h_seeds ? (int64_t)n_seeds : (int64_t)n;
  if (!d_p && count > 0 && n > 0)
    return invalid("grx_ppr: d_p is NULL");
  const bool timed = o.collect_kernel_time != 0;
  return guarded([&] {
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (n == 0 || count == 0)  // nothing to rank: nothing is written, nothing is launched
      return (int)GRX_OK;
    if (int rc = ensure_can_pull(ctx, g)) {  // the sum runs over in-entries
      last_error() = "grx_ppr: " + last_error();
      return rc;
    }
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();

    // test hook: the in-row entries one lane group sums
    const int32_t segment = (int32_t)env_or("GRX_PPR_SEGMENT", k::PPR_SEGMENT, k::PPR_SEGMENT_MIN, INT32_MAX);

    call_clock_t clock(s, timed);
    clock.start();

    long long iterations_total = 0, launches = 0;
    unsigned long long nonzero_total = 0;
    {
      const std::size_t nv = (std::size_t)n, nnz = (std::size_t)g->nnz;
      const k::csr_rows_t in = in_rows(g);
      // once per call: scale, the dangling list, the long in-rows and their items
      const std::size_t most_long = nnz / (std::size_t)segment + 1;  // a long row has more than `segment` entries
      const std::size_t most_items = 2 * most_long;                  // ceil(d / segment) < d / segment + 1 per row
      hip::device_array_t<float> scale(nv);
      hip::device_array_t<unsigned char> flags(2 * nv);
      hip::device_array_t<int32_t> dangling(nv), long_rows(most_long), first(most_long + 1), counts(2);
      hip::device_array_t<int2> items(most_items);
      clock.begin_batch();
      k::ppr_scale_kernel<<<grid_for(nv, k::PPR_BLOCK / hip::wave_size, sc), k::PPR_BLOCK, 0, s>>>(
          g->d_ap, g->d_ax, in, alpha, n, segment, scale.data(), flags.data(), flags.data() + nv);
      list_flagged(flags.data(), nv, dangling.data(), counts.data(), s);
      list_flagged(flags.data() + nv, nv, long_rows.data(), counts.data() + 1, s);
      k::ppr_items_kernel<<<1, k::PPR_BLOCK, 0, s>>>(in, long_rows.data(), counts.data() + 1, segment, first.data(),
                                                    items.data(), (int32_t)std::min<std::size_t>(most_items, INT32_MAX));
      GRX_HIP_CHECK(hipGetLastError());
      clock.end_batch();
      launches += 2;
      int32_t h_counts[2] = {0, 0}, n_items = 0;
      GRX_HIP_CHECK(hipMemcpyAsync(h_counts, counts.data(), sizeof h_counts, hipMemcpyDeviceToHost, s));
      GRX_HIP_CHECK(hipStreamSynchronize(s));
      const int32_t n_dangling = h_counts[0], n_long = h_counts[1];
      error::throw_if_exception((std::size_t)n_long > most_long, "grx_ppr: more long in-rows than nnz allows");
      if (n_long) {
        GRX_HIP_CHECK(hipMemcpyAsync(&n_items, first.data() + n_long, sizeof n_items, hipMemcpyDeviceToHost, s));
        GRX_HIP_CHECK(hipStreamSynchronize(s));
        error::throw_if_exception((std::size_t)n_items > most_items, "grx_ppr: more segments than nnz allows");
      }
      const int32_t chunks = (n_dangling + k::PPR_DANGLING_CHUNK - 1) / k::PPR_DANGLING_CHUNK;

      hip::device_array_t<k::ppr_counters_t> counters(1);
      k::ppr_counters_t* ctr = counters.data();
      k::ppr_counters_t h_ctr;

      // per vertex: p and the two give arrays, 12 L bytes; allocated once for the widest batch
      const int widest = (int)std::min<int64_t>(k::PPR_BATCH, count);
      const int L_most = widest <= 16 ? 16 : widest <= 32 ? 32 : 64;
      hip::device_array_t<float> state(3 * nv * (std::size_t)L_most);
      hip::device_array_t<float> partial(std::max<std::size_t>((std::size_t)n_items * L_most, 1));
      hip::device_array_t<float> dpart(std::max<std::size_t>((std::size_t)chunks * L_most, 1));

      for (int64_t first_seed = 0; first_seed < count; first_seed += k::PPR_BATCH) {
        const int width = (int)std::min<int64_t>(k::PPR_BATCH, count - first_seed);
        const int L = width <= 16 ? 16 : width <= 32 ? 32 : 64;
        const std::size_t words = nv * (std::size_t)L;
        k::ppr_seeds_t seeds;
        for (int i = 0; i < k::PPR_BATCH; ++i)
          seeds.v[i] = i >= width ? -1 : h_seeds ? h_seeds[first_seed + i] : (int32_t)(first_seed + i);
        // columns the batch does not use are frozen from the start and stay 0
        unsigned long long frozen = width == k::PPR_BATCH ? 0ull : ~0ull << width;
        float* p = state.data();
        float* give = state.data() + words;
        float* next = state.data() + 2 * words;
        float* out = d_p + (std::size_t)first_seed * nv;

        with_width(L, [&](auto width_tag) {
          constexpr int W = decltype(width_tag)::value;
          constexpr std::size_t rows = k::ppr_shape_t<W>::groups;
          clock.begin_batch();
          GRX_HIP_CHECK(hipMemsetAsync(p, 0, 2 * words * sizeof(float), s));  // p and the current give
          GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof *ctr, s));
          k::ppr_seed_kernel<W><<<1, k::PPR_BATCH, 0, s>>>(seeds, width, scale.data(), p, give, ctr, frozen);
          ++launches;
          int32_t t = 0;
          for (;;) {
            ++t;
            if (first_seed == 0 && t <= 64 && stats) {
              stats->frontier_slots[t - 1] = __builtin_popcountll(~frozen);
              stats->levels_recorded = t;
            }
            // a column that contracts stops long before this; NaN weights never do
            error::throw_if_exception(t > (1 << 20), "grx_ppr: no column below tol after 2^20 iterations");
            const k::ppr_state_t st{scale.data(), p, give, next, seeds, frozen, alpha, ctr};
            k::ppr_gather_kernel<W><<<odd_grid_for(nv, rows, sc), k::PPR_BLOCK, 0, s>>>(in, st, n, segment);
            ++launches;
            if (n_long) {
              k::ppr_segment_kernel<W><<<grid_for((std::size_t)n_items, rows, sc), k::PPR_BLOCK, 0, s>>>(
                  in, give, items.data(), n_items, segment, partial.data());
              k::ppr_combine_kernel<W><<<grid_for((std::size_t)n_long, rows, sc), k::PPR_BLOCK, 0, s>>>(
                  st, long_rows.data(), first.data(), n_long, partial.data());
              launches += 2;
            }
            if (chunks) {
              k::ppr_dangling_kernel<W><<<grid_for((std::size_t)chunks, rows, sc), k::PPR_BLOCK, 0, s>>>(
                  p, dangling.data(), n_dangling, dpart.data());
              ++launches;
            }
            unsigned long long* m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
              k::ppr_publish_kernel<<<1, k::PPR_BATCH, 0, s>>>(ctr, dpart.data(), chunks, W, width, t, tol, mirror, slot,
                                                              seq);
            });
            ++launches;
            frozen = m[k::PM_FROZEN];
            std::swap(give, next);
            if (~frozen == 0 || (o.max_iterations && t >= o.max_iterations))
              break;
            clock.begin_batch();
          }
          clock.begin_batch();
          k::ppr_deliver_kernel<W><<<grid_for(nv, k::PPR_TILE, sc), k::PPR_BLOCK, 0, s>>>(p, n, width, out, ctr);
          GRX_HIP_CHECK(hipGetLastError());
          clock.end_batch();
          ++launches;
        });

        // the batch's figures: every kernel that wrote them is enqueued before the copy
        GRX_HIP_CHECK(hipMemcpyAsync(&h_ctr, ctr, sizeof h_ctr, hipMemcpyDeviceToHost, s));
        GRX_HIP_CHECK(hipStreamSynchronize(s));
        int32_t longest = 0;
        for (int i = 0; i < width; ++i) {
          if (h_iterations)
            h_iterations[first_seed + i] = h_ctr.iterations[i];
          if (h_residual)
            h_residual[first_seed + i] = h_ctr.residual[i];
          longest = std::max(longest, h_ctr.iterations[i]);
          nonzero_total += h_ctr.nonzero[i];
        }
        iterations_total += longest;
      }
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();

    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->iterations = (int32_t)std::min<long long>(iterations_total, INT32_MAX);
      stats->advance_launches = (int32_t)std::min<long long>(launches, INT32_MAX);
      stats->vertices_reached = (int64_t)nonzero_total;
      stats->edges_traversed = stats->edges_expanded = (int64_t)g->nnz * (int64_t)iterations_total;
    }
    return (int)GRX_OK;
  });
}

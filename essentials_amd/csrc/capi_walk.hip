/** @file capi_walk.hip  grx_random_walk: first-order and node2vec random walks whose every draw is a
 * function of (seed, walk, step, draw index), so a walk is the same bits in every call, batch and
 * schedule (hip/kernels/walk_kernels.hxx).  No reference counterpart.  Per call: the prefix array of
 * a weighted walk (local sums, block bases, their sum), the column-sorted rows of a second-order walk
 * (the (row, column) keys of grx_graph_sorted_rows, sorted without their weights), then one walker
 * launch, one lane per walk. */
#include "capi_batch.hxx"
#include "simple_csr.hxx"

#include <gunrock/hip/kernels/walk_kernels.hxx>

#include <cmath>

using namespace essentials_amd;

namespace k = gunrock::hip::kernels;

namespace {

/// n + 1 scan inputs: the prefix blocks of row v for v < n, 0 at v == n.
struct row_blocks_t {
  const int32_t* ap;
  int32_t n;
  __host__ __device__ int32_t operator()(int32_t v) const { return v < n ? k::walk_blocks_of(ap[v + 1] - ap[v]) : 0; }
};

bool in_range(float x) { return x >= 0.125f && x <= 8.0f; }  // false for NaN

}  // namespace

extern "C" int grx_random_walk(grx_context_t ctx, grx_graph_t g, const int32_t* h_starts, int32_t n_starts,
                               int32_t length, uint64_t seed, int32_t weighted, float p, float q, int32_t* d_walks,
                               const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_random_walk: NULL argument");
  if (n_starts < 0)
    return invalid("grx_random_walk: n_starts < 0");
  if (!h_starts && n_starts != 0)
    return invalid("grx_random_walk: h_starts is NULL (every vertex) but n_starts != 0");
  for (int32_t i = 0; i < n_starts; ++i)
    if (h_starts[i] < 0 || h_starts[i] >= g->n_rows)
      return invalid("grx_random_walk: start out of range");
  if (length < 0)
    return invalid("grx_random_walk: length < 0");
  if (g->n_rows != g->n_cols)
    return invalid("grx_random_walk: the graph is not square (n_rows != n_cols)");
  if (!in_range(p) || !in_range(q))
    return invalid("grx_random_walk: p and q must be in [0.125, 8]");
  const grx_options o = effective_options(opt);
  if (o.max_iterations != 0)
    return invalid("grx_random_walk: max_iterations must be 0 (the walk's length is an argument)");
  const int32_t n = g->n_rows;
  const int64_t count = h_starts ? (int64_t)n_starts : (int64_t)n;
  if (!d_walks && count > 0 && n > 0)
    return invalid("grx_random_walk: d_walks is NULL");
  const bool timed = o.collect_kernel_time != 0;
  return guarded([&] {
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (n == 0 || count == 0)  // nobody walks: nothing is written, nothing is launched
      return (int)GRX_OK;
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();

    // test hook: the candidates of a node2vec step before the last one is taken
    const int32_t cap = (int32_t)env_or("GRX_WALK_MAX_ATTEMPTS", k::WALK_MAX_ATTEMPTS, 1, k::WALK_MAX_ATTEMPTS);

    // node2vec's acceptance ratios, float32: the largest of 1/p, 1 and 1/q is accepted always
    const float ip = 1.0f / p, iq = 1.0f / q;
    const float m = std::max(std::max(ip, 1.0f), iq);
    const bool second = !(p == 1.0f && q == 1.0f);
    // a walk that never steps picks nothing: no prefix array, no sorted rows
    const std::size_t nnz = length > 0 ? (std::size_t)g->nnz : 0;
    const bool by_weight = weighted != 0 && nnz > 0, by_class = second && length > 1 && nnz > 0;

    call_clock_t clock(s, timed);
    clock.start();
    int32_t launches = 0;
    unsigned long long h_counters[k::WC_COUNT];
    {
      hip::device_array_t<float> c(by_weight ? nnz : 0);
      hip::device_array_t<int32_t> sorted(by_class ? nnz : 0);
      hip::device_array_t<int32_t> starts(h_starts ? (std::size_t)count : 0);
      hip::device_array_t<unsigned long long> counters(k::WC_COUNT);
      GRX_HIP_CHECK(hipMemsetAsync(counters.data(), 0, k::WC_COUNT * sizeof(unsigned long long), s));
      if (h_starts)
        GRX_HIP_CHECK(hipMemcpyAsync(starts.data(), h_starts, (std::size_t)count * sizeof(int32_t),
                                     hipMemcpyHostToDevice, s));
      clock.begin_batch();
      if (by_weight) {
        // blocks of 64 entries in row order; their number is below V + nnz / 64
        error::throw_if_exception((std::size_t)n + nnz / k::WALK_PREFIX_BLOCK > (std::size_t)INT32_MAX,
                                  "grx_random_walk: more prefix blocks than int32 holds");
        hip::device_array_t<int32_t> first_block((std::size_t)n + 1);
        {
          auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int32_t>(0),
                                                     row_blocks_t{g->d_ap, n});
          const std::size_t bytes = hip::exclusive_sum_temp_bytes(in, first_block.data(), int32_t(0), (std::size_t)n + 1);
          hip::buffer_t<unsigned char> temp(bytes < 256 ? 256 : bytes);
          hip::exclusive_sum(temp.data(), bytes, in, first_block.data(), int32_t(0), (std::size_t)n + 1, s);
        }
        int32_t n_blocks = 0;
        GRX_HIP_CHECK(hipMemcpyAsync(&n_blocks, first_block.data() + n, sizeof n_blocks, hipMemcpyDeviceToHost, s));
        GRX_HIP_CHECK(hipStreamSynchronize(s));
        hip::device_array_t<float> base((std::size_t)n_blocks);
        const unsigned per_wave = 64;
        k::walk_prefix_local_kernel<<<hip::grid_for((std::size_t)n_blocks, per_wave * (k::WALK_PREFIX_THREADS / 64),
                                                    UINT32_MAX),
                                      k::WALK_PREFIX_THREADS, 0, s>>>(g->d_ap, g->d_ax, first_block.data(), n, n_blocks,
                                                                      c.data(), base.data());
        k::walk_prefix_base_kernel<<<grid_for((std::size_t)n, k::WALK_BLOCK, sc), k::WALK_BLOCK, 0, s>>>(
            first_block.data(), n, base.data());
        k::walk_prefix_apply_kernel<<<hip::grid_for((std::size_t)n_blocks, per_wave * (k::WALK_BLOCK / 64), UINT32_MAX),
                                      k::WALK_BLOCK, 0, s>>>(g->d_ap, first_block.data(), n, n_blocks, base.data(),
                                                             c.data());
        GRX_HIP_CHECK(hipGetLastError());
        launches += 3;
        GRX_HIP_CHECK(hipStreamSynchronize(s));  // the two lists go before the walker runs
      }
      if (by_class) {
        hip::buffer_t<unsigned long long> keys(nnz), keys2(nnz);
        const unsigned grid = (unsigned)sc.compute_units() * 8;
        row_col_keys_kernel<<<grid, 256, 0, s>>>(g->d_ap, g->d_aj, n, (long long)nnz, keys.data());
        GRX_HIP_CHECK(hipGetLastError());
        unsigned row_bits = 1;
        while (row_bits < 32 && ((unsigned)n - 1) >> row_bits)
          ++row_bits;
        std::size_t bytes = 0;
        GRX_HIP_CHECK(rocprim::radix_sort_keys(nullptr, bytes, keys.data(), keys2.data(), nnz, 0, 32 + row_bits, s));
        hip::buffer_t<unsigned char> temp(bytes < 256 ? 256 : bytes);  // never null: rocPRIM would only size
        GRX_HIP_CHECK(rocprim::radix_sort_keys(temp.data(), bytes, keys.data(), keys2.data(), nnz, 0, 32 + row_bits, s));
        keys_to_cols_kernel<<<grid, 256, 0, s>>>(keys2.data(), (long long)nnz, sorted.data());
        GRX_HIP_CHECK(hipGetLastError());
        launches += 2;
        GRX_HIP_CHECK(hipStreamSynchronize(s));  // the keys go before the walker runs
      }
      const k::walk_args_t a{g->d_ap,  g->d_aj, c.data(), sorted.data(), h_starts ? starts.data() : nullptr,
                             count,    length,  seed,     ip / m,        1.0f / m,
                             iq / m,   cap,     d_walks,  counters.data()};
      const unsigned grid = hip::grid_for((std::size_t)count, k::WALK_BLOCK, UINT32_MAX);
      if (by_weight && by_class)
        k::walk_kernel<true, true><<<grid, k::WALK_BLOCK, 0, s>>>(a);
      else if (by_weight)
        k::walk_kernel<true, false><<<grid, k::WALK_BLOCK, 0, s>>>(a);
      else if (by_class)
        k::walk_kernel<false, true><<<grid, k::WALK_BLOCK, 0, s>>>(a);
      else
        k::walk_kernel<false, false><<<grid, k::WALK_BLOCK, 0, s>>>(a);
      GRX_HIP_CHECK(hipGetLastError());
      clock.end_batch();
      ++launches;
      GRX_HIP_CHECK(hipMemcpyAsync(h_counters, counters.data(), sizeof h_counters, hipMemcpyDeviceToHost, s));
      GRX_HIP_CHECK(hipStreamSynchronize(s));
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();

    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->advance_launches = launches;
      stats->iterations = (int32_t)h_counters[k::WC_LONGEST];
      stats->vertices_reached = (int64_t)h_counters[k::WC_FULL];
      stats->edges_traversed = (int64_t)h_counters[k::WC_STEPS];
      stats->edges_expanded = (int64_t)h_counters[k::WC_ATTEMPTS];
      stats->levels_recorded = std::min<int32_t>(stats->iterations, k::WALK_LEVELS);
      // walks that took step t: those that took t steps or more
      unsigned long long took = 0;
      for (int t = k::WALK_LEVELS; t >= 1; --t) {
        took += h_counters[k::WC_TOOK + t];
        stats->frontier_slots[t - 1] = (int64_t)took;
      }
    }
    return (int)GRX_OK;
  });
}

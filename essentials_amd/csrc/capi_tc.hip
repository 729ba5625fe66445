/** @file capi_tc.hip  grx_tc == gunrock::tc::run (reference algorithms/tc.hxx) on the simple
 * undirected graph under a symmetric CSR: a degree-oriented, sorted, deduplicated copy L is built
 * per call and every triangle is found once, at its lowest-ranked vertex (hip/kernels/tc_kernels.hxx). */
#include "capi_batch.hxx"

#include <gunrock/hip/kernels/tc_kernels.hxx>

#include <cstring>

using namespace essentials_amd;

namespace {

namespace k = gunrock::hip::kernels;

/// n + 1 scan inputs: count[p] for p < n, 0 at p == n.
struct padded_t {
  const int32_t* count;
  int32_t n;
  __host__ __device__ int32_t operator()(int32_t p) const { return p < n ? count[p] : 0; }
};

/// Size class of row u of L.
struct class_key_t {
  const int32_t* lap;
  int32_t b[4];
  __host__ __device__ unsigned operator()(int32_t u) const { return k::tc_class_of(lap[u + 1] - lap[u], b); }
};

/// Exclusive scan of count[0, n) into out[0, n] (out[n] = the sum).
void scan_counts(const int32_t* count, int32_t n, int32_t* out, hip::device_array_t<unsigned char>& temp,
                 hipStream_t s) {
  auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int32_t>(0), padded_t{count, n});
  const std::size_t bytes = hip::exclusive_sum_temp_bytes(in, out, int32_t(0), (std::size_t)n + 1);
  if (temp.size() < bytes)
    temp.resize(bytes);
  hip::exclusive_sum(temp.data(), bytes, in, out, int32_t(0), (std::size_t)n + 1, s);
}

}  // namespace

extern "C" int grx_tc(grx_context_t ctx, grx_graph_t g, int64_t* d_vertex_triangles, uint64_t* h_triangles,
                      const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_tc: NULL argument");
  if (!d_vertex_triangles && !h_triangles)
    return invalid("grx_tc: both outputs are NULL");
  if (g->n_rows != g->n_cols)
    return invalid("grx_tc: the graph is not square (n_rows != n_cols)");
  const bool timed = opt && opt->collect_kernel_time;
  return guarded([&] {
    if (int rc = require_symmetric(ctx, g, "grx_tc", "triangle counting"))
      return rc;
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();
    const int32_t n = g->n_rows;
    const std::size_t nnz = (std::size_t)g->nnz;
    if (stats)
      std::memset(stats, 0, sizeof *stats);

    int32_t lds_ids = k::TC_LDS_IDS;  // staging capacity of the workgroup path
    {
      int dev = 0, max_lds = 0;
      GRX_HIP_CHECK(hipGetDevice(&dev));
      GRX_HIP_CHECK(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
      const int fit = (max_lds - 1024) / k::TC_SLOT_BYTES;  // the static part stays below 1 KB
      lds_ids = std::min(lds_ids, fit);
      lds_ids = (int32_t)env_or("GRX_TC_LDS_IDS", lds_ids, 1, lds_ids);  // test hook: lower the capacity
    }

    call_clock_t clock(s, timed);
    clock.start();
    if (d_vertex_triangles && n)
      GRX_HIP_CHECK(hipMemsetAsync(d_vertex_triangles, 0, (std::size_t)n * sizeof(int64_t), s));

    unsigned long long h_totals[2] = {0, 0};
    long long m = 0;  // entries of L: the simple undirected edges that are not self loops
    {
      // 1. L: orient, sort, deduplicate
      hip::device_array_t<int32_t> count((std::size_t)std::max(n, 1)), K((std::size_t)n + 1),
          lap((std::size_t)n + 1);
      hip::device_array_t<unsigned char> temp(256);
      int bits = 1;
      while (bits < 31 && (int64_t(1) << bits) <= (int64_t)n)
        ++bits;  // n < 2^bits: every column fits the low bits of a key
      const unsigned grid = grid_for((std::size_t)std::max(n, 1), k::TC_BLOCK / hip::wave_size, sc);
      int32_t kept = 0;
      if (n) {
        k::tc_orient_kernel<false><<<grid, k::TC_BLOCK, 0, s>>>(g->d_ap, g->d_aj, n, count.data(), nullptr,
                                                                nullptr, bits);
        GRX_HIP_CHECK(hipGetLastError());
        scan_counts(count.data(), n, K.data(), temp, s);
        GRX_HIP_CHECK(hipMemcpyAsync(&kept, K.data() + n, sizeof kept, hipMemcpyDeviceToHost, s));
        GRX_HIP_CHECK(hipStreamSynchronize(s));
      }
      hip::device_array_t<int32_t> laj((std::size_t)std::max(kept, 1));
      if (kept) {
        hip::device_array_t<unsigned long long> keys((std::size_t)kept), sorted((std::size_t)kept);
        k::tc_orient_kernel<true><<<grid, k::TC_BLOCK, 0, s>>>(g->d_ap, g->d_aj, n, nullptr, K.data(),
                                                               keys.data(), bits);
        GRX_HIP_CHECK(hipGetLastError());
        std::size_t bytes = 0;
        GRX_HIP_CHECK(rocprim::radix_sort_keys(nullptr, bytes, keys.data(), sorted.data(), (std::size_t)kept, 0,
                                               2 * bits, s));
        if (temp.size() < bytes)
          temp.resize(bytes);
        GRX_HIP_CHECK(rocprim::radix_sort_keys(temp.data(), bytes, keys.data(), sorted.data(), (std::size_t)kept,
                                               0, 2 * bits, s));
        const unsigned long long col_mask = (1ull << bits) - 1;
        k::tc_distinct_kernel<false><<<grid, k::TC_BLOCK, 0, s>>>(sorted.data(), K.data(), n, count.data(),
                                                                  nullptr, nullptr, col_mask);
        GRX_HIP_CHECK(hipGetLastError());
        scan_counts(count.data(), n, lap.data(), temp, s);
        k::tc_distinct_kernel<true><<<grid, k::TC_BLOCK, 0, s>>>(sorted.data(), K.data(), n, nullptr,
                                                                 lap.data(), laj.data(), col_mask);
        GRX_HIP_CHECK(hipGetLastError());
      } else if (n) {
        GRX_HIP_CHECK(hipMemsetAsync(lap.data(), 0, ((std::size_t)n + 1) * sizeof(int32_t), s));
      }

      // 2. rows of L by size class (stable: ascending ids within a class)
      hip::device_array_t<int32_t> rows((std::size_t)std::max(n, 1));
      hip::device_array_t<unsigned> classes((std::size_t)std::max(n, 1));
      hip::device_array_t<int32_t> starts(k::TC_CLASSES + 2);
      std::vector<int32_t> h_starts(k::TC_CLASSES + 2, 0);
      const int32_t b[4] = {std::min(k::TC_SMALL, lds_ids), std::min(k::TC_WAVE, lds_ids),
                            std::min(k::TC_MEDIUM, lds_ids), lds_ids};
      if (kept) {
        auto key_it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int32_t>(0),
                                                       class_key_t{lap.data(), {b[0], b[1], b[2], b[3]}});
        std::size_t bytes = 0;
        GRX_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, key_it, classes.data(),
                                                rocprim::make_counting_iterator<int32_t>(0), rows.data(),
                                                (std::size_t)n, 0, 3, s));
        if (temp.size() < bytes)
          temp.resize(bytes);
        GRX_HIP_CHECK(rocprim::radix_sort_pairs(temp.data(), bytes, key_it, classes.data(),
                                                rocprim::make_counting_iterator<int32_t>(0), rows.data(),
                                                (std::size_t)n, 0, 3, s));
        k::tc_class_starts_kernel<<<1, 64, 0, s>>>(classes.data(), n, starts.data());
        GRX_HIP_CHECK(hipGetLastError());
        GRX_HIP_CHECK(hipMemcpyAsync(starts.data() + k::TC_CLASSES + 1, lap.data() + n, sizeof(int32_t),
                                     hipMemcpyDeviceToDevice, s));
        GRX_HIP_CHECK(hipMemcpyAsync(h_starts.data(), starts.data(), h_starts.size() * sizeof(int32_t),
                                     hipMemcpyDeviceToHost, s));
        GRX_HIP_CHECK(hipStreamSynchronize(s));
      }
      m = h_starts[k::TC_CLASSES + 1];
      auto rows_of = [&](int c) { return h_starts[c + 1] - h_starts[c]; };
      const int32_t* rows_at[k::TC_CLASSES];
      for (int c = 0; c < k::TC_CLASSES; ++c)
        rows_at[c] = rows.data() + h_starts[c];

      // 3. counting: the widest rows first
      hip::device_array_t<unsigned long long> totals(2);
      GRX_HIP_CHECK(hipMemsetAsync(totals.data(), 0, sizeof h_totals, s));
      auto* counts = reinterpret_cast<unsigned long long*>(d_vertex_triangles);
      hip::device_array_t<int32_t> ws(rows_of(5) ? 3 * (std::size_t)m : 0);
      clock.begin_batch();
      if (int32_t r = rows_of(5)) {
        k::tc_block_kernel<false><<<grid_for((std::size_t)r, 1, sc), k::TC_BLOCK, 0, s>>>(
            lap.data(), laj.data(), rows_at[5], r, 0, ws.data(), m, counts, totals.data());
        GRX_HIP_CHECK(hipGetLastError());
      }
      if (int32_t r = rows_of(4)) {
        // the longest staged row sizes the LDS image
        const int32_t cap = (int32_t)std::min<unsigned long long>(reduce_max_degree(lap.data(), n), (unsigned long long)b[3]);
        const std::size_t lds = (std::size_t)cap * k::TC_SLOT_BYTES;
        GRX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k::tc_block_kernel<true>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        k::tc_block_kernel<true><<<grid_for((std::size_t)r, 1, sc), k::TC_BLOCK, lds, s>>>(
            lap.data(), laj.data(), rows_at[4], r, cap, nullptr, m, counts, totals.data());
        GRX_HIP_CHECK(hipGetLastError());
      }
      if (int32_t r = rows_of(3)) {
        k::tc_block_kernel<true><<<grid_for((std::size_t)r, 1, sc), k::TC_BLOCK,
                                   (std::size_t)b[2] * k::TC_SLOT_BYTES, s>>>(
            lap.data(), laj.data(), rows_at[3], r, b[2], nullptr, m, counts, totals.data());
        GRX_HIP_CHECK(hipGetLastError());
      }
      if (int32_t r = rows_of(2)) {
        k::tc_group_kernel<k::TC_WAVE><<<grid_for((std::size_t)r, k::TC_BLOCK / k::TC_WAVE, sc), k::TC_BLOCK, 0, s>>>(
            lap.data(), laj.data(), rows_at[2], r, counts, totals.data());
        GRX_HIP_CHECK(hipGetLastError());
      }
      if (int32_t r = rows_of(1)) {
        k::tc_group_kernel<k::TC_SMALL><<<grid_for((std::size_t)r, k::TC_BLOCK / k::TC_SMALL, sc), k::TC_BLOCK, 0,
                                          s>>>(lap.data(), laj.data(), rows_at[1], r, counts, totals.data());
        GRX_HIP_CHECK(hipGetLastError());
      }
      clock.end_batch();
      GRX_HIP_CHECK(hipMemcpyAsync(h_totals, totals.data(), sizeof h_totals, hipMemcpyDeviceToHost, s));
      clock.stop_and_wait();
    }
    // the key buffers are large and of no use to the operators: do not park them
    hip::block_cache_t::instance().trim();

    if (h_triangles)
      *h_triangles = (uint64_t)h_totals[0];
    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->iterations = 1;
      stats->edges_traversed = (int64_t)m;
      stats->edges_expanded = (int64_t)h_totals[1];
    }
    return (int)GRX_OK;
  });
}

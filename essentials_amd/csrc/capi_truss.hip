/** @file capi_truss.hip  grx_truss: the trussness of every edge of the simple undirected graph under a
 * symmetric CSR.  Per call: the simple sorted copy with an id per edge, the support of every edge by
 * listing every triangle once on the degree-oriented copy, a peel on an append-only queue of edges, and
 * the scatter to the caller's entries (hip/kernels/truss_kernels.hxx).  The reference has no k-truss. */
#include "capi_batch.hxx"
#include "simple_csr.hxx"

#include <gunrock/hip/kernels/truss_kernels.hxx>

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

/// Size class of row u of the oriented copy.
struct class_key_t {
  const int32_t* lap;
  int32_t b[4];
  __host__ __device__ unsigned operator()(int32_t u) const { return k::truss_class_of(lap[u + 1] - lap[u], b); }
};

}  // namespace

extern "C" int grx_truss(grx_context_t ctx, grx_graph_t g, int32_t* d_truss, int32_t* h_max_truss,
                         const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_truss: NULL argument");
  if (!d_truss && !h_max_truss)
    return invalid("grx_truss: both outputs are NULL");
  if (g->n_rows != g->n_cols)
    return invalid("grx_truss: the graph is not square (n_rows != n_cols)");
  if (opt && opt->max_iterations != 0)
    return invalid("grx_truss: max_iterations must be 0 (the peel runs until no edge is left)");
  const bool timed = opt && opt->collect_kernel_time;
  return guarded([&] {
    const int32_t n = g->n_rows;
    const std::size_t nnz = (std::size_t)g->nnz;
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (h_max_truss)
      *h_max_truss = 0;
    if (n == 0 || nnz == 0)  // no entry: nothing to write
      return (int)GRX_OK;
    if (int rc = require_symmetric(ctx, g, "grx_truss", "k-truss decomposition"))
      return rc;
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();

    // test hooks: the probes a generation may have to stay in the one-workgroup kernel (0 sends
    // every generation to the wide kernel), and the staging capacity of the support's workgroup path
    const unsigned long long narrow_edges =
        (unsigned long long)env_or("GRX_TRUSS_NARROW_EDGES", k::TR_NARROW_EDGES, 0, 1ll << 62);
    int32_t lds_ids = k::TR_LDS_IDS;
    {
      int dev = 0, max_lds = 0;
      GRX_HIP_CHECK(hipGetDevice(&dev));
      GRX_HIP_CHECK(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
      const int fit = (max_lds - 1024) / k::TR_SLOT_BYTES;  // the static part stays below 1 KB
      lds_ids = std::min(lds_ids, fit);
      lds_ids = (int32_t)env_or("GRX_TRUSS_LDS_IDS", lds_ids, 1, lds_ids);
    }

    call_clock_t clock(s, timed);
    clock.start();

    int32_t max_truss = 0, levels = 0, launches = 0;
    long long m = 0;
    unsigned long long probes = 0;
    float phase_ms[3] = {0, 0, 0};
    {
      const unsigned grid = (unsigned)sc.compute_units() * 8;
      const unsigned row_grid = grid_for((std::size_t)n, k::TR_BLOCK / hip::wave_size, sc);
      hip::device_array_t<unsigned char> temp(256);
      auto need = [&](std::size_t bytes) {
        if (temp.size() < bytes)
          temp.resize(bytes);
      };

      // 1. the simple sorted copy S: sort the (row, column) keys, keep the first of every run that is
      // no self loop
      clock.begin_batch();
      hip::device_array_t<int32_t> sp((std::size_t)n + 1);
      int kept = 0;
      hip::device_array_t<int32_t> sj;
      {
        hip::device_array_t<unsigned long long> keys(nnz), sorted(nnz);
        hip::device_array_t<int> at(nnz + 1);
        row_col_keys_kernel<<<grid, 256, 0, s>>>(g->d_ap, g->d_aj, n, (long long)nnz, keys.data());
        GRX_HIP_CHECK(hipGetLastError());
        int bits = 1;
        while (bits < 31 && (int64_t(1) << bits) <= (int64_t)n)
          ++bits;  // n < 2^bits: no row above bit 32 + bits
        std::size_t bytes = 0;
        GRX_HIP_CHECK(rocprim::radix_sort_keys(nullptr, bytes, keys.data(), sorted.data(), nnz, 0, 32 + bits, s));
        auto keep = rocprim::make_transform_iterator(rocprim::make_counting_iterator<long long>(0),
                                                     simple_keep_t{sorted.data(), (long long)nnz});
        need(std::max(bytes, hip::exclusive_sum_temp_bytes(keep, at.data(), 0, nnz + 1)));
        bytes = temp.size();
        GRX_HIP_CHECK(rocprim::radix_sort_keys(temp.data(), bytes, keys.data(), sorted.data(), nnz, 0, 32 + bits, s));
        hip::exclusive_sum(temp.data(), temp.size(), keep, at.data(), 0, nnz + 1, s);
        GRX_HIP_CHECK(hipMemcpyAsync(&kept, at.data() + nnz, sizeof kept, hipMemcpyDeviceToHost, s));
        GRX_HIP_CHECK(hipStreamSynchronize(s));
        sj.resize((std::size_t)std::max(kept, 1));
        k::truss_cols_kernel<<<grid, k::TR_BLOCK, 0, s>>>(sorted.data(), at.data(), (long long)nnz, sj.data());
        simple_offsets_kernel<<<grid, 256, 0, s>>>(g->d_ap, at.data(), n, sp.data());
        GRX_HIP_CHECK(hipGetLastError());
        launches += 5;
        GRX_HIP_CHECK(hipStreamSynchronize(s));  // the key buffers go before the edge arrays come
      }
      const std::size_t m2 = (std::size_t)kept;

      // ... and its edge ids: the entries above the diagonal, in order
      hip::device_array_t<int32_t> ebase((std::size_t)n + 1), eid(std::max<std::size_t>(m2, 1));
      hip::device_array_t<int32_t> eu, ev;
      if (m2) {
        hip::device_array_t<int32_t> upper((std::size_t)n);
        k::truss_upper_kernel<<<grid_for((std::size_t)n, k::TR_BLOCK, sc), k::TR_BLOCK, 0, s>>>(sp.data(), sj.data(), n,
                                                                                              upper.data());
        GRX_HIP_CHECK(hipGetLastError());
        auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int32_t>(0),
                                                   padded_t{upper.data(), n});
        need(hip::exclusive_sum_temp_bytes(in, ebase.data(), int32_t(0), (std::size_t)n + 1));
        hip::exclusive_sum(temp.data(), temp.size(), in, ebase.data(), int32_t(0), (std::size_t)n + 1, s);
        int32_t edges = 0;
        GRX_HIP_CHECK(hipMemcpyAsync(&edges, ebase.data() + n, sizeof edges, hipMemcpyDeviceToHost, s));
        GRX_HIP_CHECK(hipStreamSynchronize(s));
        m = edges;
        error::throw_if_exception(2 * (std::size_t)m != m2, "grx_truss: the simple graph is not symmetric");
        eu.resize((std::size_t)m);
        ev.resize((std::size_t)m);
        k::truss_edge_ids_kernel<<<row_grid, k::TR_BLOCK, 0, s>>>(sp.data(), sj.data(), ebase.data(), n, (int32_t)m,
                                                                  eid.data(), eu.data(), ev.data());
        GRX_HIP_CHECK(hipGetLastError());
        launches += 3;
      }
      clock.end_batch();
      if (timed)
        phase_ms[0] = clock.kernel_ms();

      if (m == 0) {  // self loops only: every entry carries 0
        if (d_truss)
          GRX_HIP_CHECK(hipMemsetAsync(d_truss, 0, nnz * sizeof(int32_t), s));
        clock.stop_and_wait();
      } else {
        const k::truss_graph_t G{sp.data(), sj.data(), eid.data(), eu.data(), ev.data(), n, (int32_t)m};
        hip::device_array_t<int32_t> support((std::size_t)m), stamp((std::size_t)m), truss((std::size_t)m),
            queue((std::size_t)m);
        const k::truss_state_t st{support.data(), stamp.data(), truss.data()};
        hip::device_array_t<k::truss_counters_t> counters(1);
        hip::device_array_t<unsigned long long> total(1);
        k::truss_counters_t* ctr = counters.data();
        GRX_HIP_CHECK(hipMemsetAsync(support.data(), 0, (std::size_t)m * sizeof(int32_t), s));
        GRX_HIP_CHECK(hipMemsetAsync(stamp.data(), 0x7f, (std::size_t)m * sizeof(int32_t), s));  // TR_ALIVE
        GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof *ctr, s));
        GRX_HIP_CHECK(hipMemsetAsync(&ctr->next_k, 0xff, sizeof ctr->next_k, s));  // TR_NONE
        GRX_HIP_CHECK(hipMemsetAsync(total.data(), 0, sizeof(unsigned long long), s));

        // 2. support: L, the degree-oriented copy of S with the edge id of every entry; its rows by
        // size class (stable: ascending ids within a class); every triangle once, the widest rows first
        {
          clock.begin_batch();
          hip::device_array_t<int32_t> count((std::size_t)n), lap((std::size_t)n + 1), laj((std::size_t)m),
              leid((std::size_t)m);
          k::truss_orient_kernel<false><<<row_grid, k::TR_BLOCK, 0, s>>>(G.sp, G.sj, G.eid, n, count.data(), nullptr,
                                                                        nullptr, nullptr);
          GRX_HIP_CHECK(hipGetLastError());
          auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int32_t>(0),
                                                     padded_t{count.data(), n});
          need(hip::exclusive_sum_temp_bytes(in, lap.data(), int32_t(0), (std::size_t)n + 1));
          hip::exclusive_sum(temp.data(), temp.size(), in, lap.data(), int32_t(0), (std::size_t)n + 1, s);
          k::truss_orient_kernel<true><<<row_grid, k::TR_BLOCK, 0, s>>>(G.sp, G.sj, G.eid, n, nullptr, lap.data(),
                                                                       laj.data(), leid.data());
          GRX_HIP_CHECK(hipGetLastError());
          launches += 3;

          hip::device_array_t<int32_t> rows((std::size_t)n);
          hip::device_array_t<unsigned> classes((std::size_t)n);
          hip::device_array_t<int32_t> starts(k::TR_CLASSES + 1);
          std::vector<int32_t> h_starts(k::TR_CLASSES + 1, 0);
          const int32_t b[4] = {std::min(k::TR_SMALL, lds_ids), std::min(k::TR_WAVE, lds_ids),
                                std::min(k::TR_MEDIUM, lds_ids), lds_ids};
          auto key_it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int32_t>(0),
                                                         class_key_t{lap.data(), {b[0], b[1], b[2], b[3]}});
          std::size_t bytes = 0;
          GRX_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, key_it, classes.data(),
                                                  rocprim::make_counting_iterator<int32_t>(0), rows.data(),
                                                  (std::size_t)n, 0, 3, s));
          if (temp.size() < bytes) {
            GRX_HIP_CHECK(hipStreamSynchronize(s));  // the scan above still reads it
            temp.resize(bytes);
          }
          bytes = temp.size();
          GRX_HIP_CHECK(rocprim::radix_sort_pairs(temp.data(), bytes, key_it, classes.data(),
                                                  rocprim::make_counting_iterator<int32_t>(0), rows.data(),
                                                  (std::size_t)n, 0, 3, s));
          k::truss_class_starts_kernel<<<1, 64, 0, s>>>(classes.data(), n, starts.data());
          GRX_HIP_CHECK(hipGetLastError());
          GRX_HIP_CHECK(hipMemcpyAsync(h_starts.data(), starts.data(), h_starts.size() * sizeof(int32_t),
                                       hipMemcpyDeviceToHost, s));
          GRX_HIP_CHECK(hipStreamSynchronize(s));
          launches += 2;
          auto rows_of = [&](int c) { return h_starts[c + 1] - h_starts[c]; };
          auto rows_at = [&](int c) { return rows.data() + h_starts[c]; };
          hip::device_array_t<int32_t> ws(rows_of(5) ? 3 * (std::size_t)m : 0);
          if (int32_t r = rows_of(5)) {
            k::truss_support_block_kernel<false><<<grid_for((std::size_t)r, 1, sc), k::TR_BLOCK, 0, s>>>(
                lap.data(), laj.data(), leid.data(), rows_at(5), r, 0, ws.data(), (int64_t)m, st.support, total.data());
            GRX_HIP_CHECK(hipGetLastError());
            ++launches;
          }
          if (int32_t r = rows_of(4)) {
            // the longest staged row sizes the LDS image
            const int32_t cap =
                (int32_t)std::min<unsigned long long>(reduce_max_degree(lap.data(), n), (unsigned long long)b[3]);
            const std::size_t lds = (std::size_t)cap * k::TR_SLOT_BYTES;
            GRX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k::truss_support_block_kernel<true>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            k::truss_support_block_kernel<true><<<grid_for((std::size_t)r, 1, sc), k::TR_BLOCK, lds, s>>>(
                lap.data(), laj.data(), leid.data(), rows_at(4), r, cap, nullptr, (int64_t)m, st.support, total.data());
            GRX_HIP_CHECK(hipGetLastError());
            ++launches;
          }
          if (int32_t r = rows_of(3)) {
            k::truss_support_block_kernel<true>
                <<<grid_for((std::size_t)r, 1, sc), k::TR_BLOCK, (std::size_t)b[2] * k::TR_SLOT_BYTES, s>>>(
                    lap.data(), laj.data(), leid.data(), rows_at(3), r, b[2], nullptr, (int64_t)m, st.support,
                    total.data());
            GRX_HIP_CHECK(hipGetLastError());
            ++launches;
          }
          if (int32_t r = rows_of(2)) {
            k::truss_support_group_kernel<k::TR_WAVE>
                <<<grid_for((std::size_t)r, k::TR_BLOCK / k::TR_WAVE, sc), k::TR_BLOCK, 0, s>>>(
                    lap.data(), laj.data(), leid.data(), rows_at(2), r, st.support, total.data());
            GRX_HIP_CHECK(hipGetLastError());
            ++launches;
          }
          if (int32_t r = rows_of(1)) {
            k::truss_support_group_kernel<k::TR_SMALL>
                <<<grid_for((std::size_t)r, k::TR_BLOCK / k::TR_SMALL, sc), k::TR_BLOCK, 0, s>>>(
                    lap.data(), laj.data(), leid.data(), rows_at(1), r, st.support, total.data());
            GRX_HIP_CHECK(hipGetLastError());
            ++launches;
          }
          clock.end_batch();
          GRX_HIP_CHECK(hipMemcpyAsync(&probes, total.data(), sizeof probes, hipMemcpyDeviceToHost, s));
          GRX_HIP_CHECK(hipStreamSynchronize(s));  // L and the workspace go before the peel starts
        }
        if (timed)
          phase_ms[1] = clock.kernel_ms() - phase_ms[0];

        // 3. peel: per level one seed scan, then generations until the queue is empty; the hand-off
        // that ends a batch is the narrow kernel's last act
        const unsigned scan_grid = grid_for((std::size_t)m, k::TR_BLOCK, sc);
        unsigned long long* mir = nullptr;
        int32_t level = 2;
        auto narrow = [&](int advance) {
          mir = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
            k::truss_narrow_kernel<<<1, k::TR_NARROW_BLOCK, 0, s>>>(G, st, queue.data(), level, advance, narrow_edges,
                                                                    ctr, mirror, slot, seq);
          });
          ++launches;
        };
        // every level above the first is named by a support some edge had: at most m + 1 trips
        for (unsigned long long queued_before = 0;;) {
          clock.begin_batch();
          k::truss_seed_kernel<<<scan_grid, k::TR_BLOCK, 0, s>>>(G, st, level, queue.data(), ctr);
          ++launches;
          narrow(0);
          run_generations(
              sc, clock, mir, k::TR_BLOCK, false, launches,
              [&](int32_t head, int32_t tail, int32_t chunk, unsigned wide_grid) {
                k::truss_wide_kernel<<<wide_grid, k::TR_BLOCK, 0, s>>>(G, st, queue.data(), head, tail, chunk, level,
                                                                       (int)mir[k::TR_GEN], ctr);
              },
              [](unsigned) {}, [&] { narrow(1); });
          // the smallest support seen above the floor may belong to an edge that left later in the
          // level: then the level it names is empty and its own scan names the next one exactly
          if (mir[k::GQ_TAIL] > queued_before) {
            ++levels;
            max_truss = level;
            queued_before = mir[k::GQ_TAIL];
          }
          if ((unsigned)mir[k::TR_NEXT_K] == k::TR_NONE)
            break;
          level = (int32_t)mir[k::TR_NEXT_K];
        }
        probes += mir[k::GQ_EDGES];

        // 4. the answer to the caller's entries
        if (d_truss) {
          clock.begin_batch();
          k::truss_scatter_kernel<<<row_grid, k::TR_BLOCK, 0, s>>>(g->d_ap, g->d_aj, G, st.truss, d_truss);
          GRX_HIP_CHECK(hipGetLastError());
          ++launches;
          clock.end_batch();
        }
        clock.stop_and_wait();
        if (timed)
          phase_ms[2] = clock.kernel_ms() - phase_ms[0] - phase_ms[1];
      }
    }
    // the key buffers and the edge arrays are large and of no use to the operators: do not park them
    hip::block_cache_t::instance().trim();

    if (h_max_truss)
      *h_max_truss = max_truss;
    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->iterations = levels;
      stats->advance_launches = launches;
      stats->edges_traversed = (int64_t)m;
      stats->edges_expanded = (int64_t)probes;
      if (timed) {
        stats->levels_recorded = 3;
        for (int p = 0; p < 3; ++p)
          stats->frontier_slots[p] = (int64_t)(phase_ms[p] * 1000.0f + 0.5f);
      }
    }
    return (int)GRX_OK;
  });
}

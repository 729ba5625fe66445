/** @file capi_spgemm.hip  grx_spgemm: C = A * B as a new owning handle.  Two-phase Gustavson with the
 * rows binned by size twice -- by their bound for the symbolic phase, by their exact length for the
 * numeric one -- and accumulated in LDS (hip/kernels/spgemm_kernels.hxx).  Not a port of the
 * reference's algorithms/spgemm.hxx, whose numeric pass indexes a row by column id. */
#include "capi_batch.hxx"

#include <gunrock/hip/kernels/spgemm_kernels.hxx>

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

/// Size class of row i: by size[i] entries (bound or exact) and products[i] products.
struct class_key_t {
  const int32_t* size;
  const unsigned long long* products;
  int32_t b[3];
  int32_t small_products;
  __host__ __device__ unsigned operator()(int32_t i) const {
    return k::spgemm_class_of(size[i], products[i], b, small_products);
  }
};

int32_t pow2_floor(long long x) {
  int32_t p = 1;
  while (2ll * p <= x)
    p <<= 1;
  return p;
}

/// The rows of one phase by class, and the launches of that phase.
struct phase_t {
  gcuda::standard_context_t& sc;
  hipStream_t s;
  int32_t n;
  hip::device_array_t<int32_t> rows;
  hip::device_array_t<unsigned> classes;
  hip::device_array_t<int32_t> starts;
  hip::device_array_t<unsigned char>& temp;
  std::vector<int32_t> h_starts;

  phase_t(gcuda::standard_context_t& c, int32_t n_rows, hip::device_array_t<unsigned char>& t)
      : sc(c), s(c.stream()), n(n_rows), rows((std::size_t)n_rows), classes((std::size_t)n_rows),
        starts(k::SG_CLASSES + 1), temp(t), h_starts(k::SG_CLASSES + 1, 0) {}

  /// Stable sort of the row ids by class (ascending ids within a class); waits for the starts.
  void bin(const class_key_t& key) {
    auto key_it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int32_t>(0), key);
    std::size_t bytes = 0;
    GRX_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, key_it, classes.data(),
                                            rocprim::make_counting_iterator<int32_t>(0), rows.data(),
                                            (std::size_t)n, 0, 3, s));
    if (temp.size() < bytes)
      temp.resize(bytes);
    GRX_HIP_CHECK(rocprim::radix_sort_pairs(temp.data(), bytes, key_it, classes.data(),
                                            rocprim::make_counting_iterator<int32_t>(0), rows.data(),
                                            (std::size_t)n, 0, 3, s));
    k::spgemm_class_starts_kernel<<<1, 64, 0, s>>>(classes.data(), n, starts.data());
    GRX_HIP_CHECK(hipGetLastError());
    GRX_HIP_CHECK(hipMemcpyAsync(h_starts.data(), starts.data(), h_starts.size() * sizeof(int32_t),
                                 hipMemcpyDeviceToHost, s));
    GRX_HIP_CHECK(hipStreamSynchronize(s));
  }
  int32_t rows_of(int c) const { return h_starts[c + 1] - h_starts[c]; }
  const int32_t* rows_at(int c) const { return rows.data() + h_starts[c]; }
};

/// Waits for the stream when it goes out of scope.  Declared AFTER a call's workspace, so that it
/// runs before the workspace is released, on every way out: a released block of 1 MiB or more is
/// parked, and another host thread's call may take it while this call's kernels still read it.
struct drain_t {
  hipStream_t s;
  ~drain_t() { (void)hipStreamSynchronize(s); }
};

/// What the kernels of both phases read.
struct operands_t {
  const int32_t *ap, *aj;
  const float* ax;
  const int32_t *bp, *bj;
  const float* bx;
  int32_t n_cols;
};

/// One phase's kernels, the widest rows first.  slots: the workgroup table's capacity;
/// tile: columns of a dense tile; returns the launches.
template <bool NUMERIC>
int32_t launch_phase(const phase_t& p, const operands_t& o, const int32_t* size, int32_t slots, int32_t tile,
                     int32_t* count, const int32_t* cp, int32_t* cj, float* cx) {
  const hipStream_t s = p.s;
  int32_t launches = 0;
  const std::size_t slot_bytes = NUMERIC ? 8 : 4;
  if (int32_t r = p.rows_of(5)) {
    const std::size_t lds = (std::size_t)tile / 8 + (NUMERIC ? (std::size_t)tile * 4 : 0);
    GRX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k::spgemm_dense_kernel<NUMERIC>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    k::spgemm_dense_kernel<NUMERIC><<<grid_for((std::size_t)r, 1, p.sc), k::SG_BLOCK, lds, s>>>(
        o.ap, o.aj, o.ax, o.bp, o.bj, o.bx, p.rows_at(5), r, o.n_cols, tile, count, cp, cj, cx);
    GRX_HIP_CHECK(hipGetLastError());
    ++launches;
  }
  for (int c = 4; c >= 3; --c)
    if (int32_t r = p.rows_of(c)) {
      const int32_t cap = c == 4 ? slots : std::min(slots, 2 * k::SG_MEDIUM);
      const std::size_t lds = (std::size_t)cap * slot_bytes;
      GRX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k::spgemm_block_kernel<NUMERIC>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      k::spgemm_block_kernel<NUMERIC><<<grid_for((std::size_t)r, 1, p.sc), k::SG_BLOCK, lds, s>>>(
          o.ap, o.aj, o.ax, o.bp, o.bj, o.bx, p.rows_at(c), r, size, cap, count, cp, cj, cx);
      GRX_HIP_CHECK(hipGetLastError());
      ++launches;
    }
  if (int32_t r = p.rows_of(2)) {
    k::spgemm_group_kernel<hip::wave_size, NUMERIC>
        <<<grid_for((std::size_t)r, k::SG_BLOCK / hip::wave_size, p.sc), k::SG_BLOCK, 0, s>>>(
            o.ap, o.aj, o.ax, o.bp, o.bj, o.bx, p.rows_at(2), r, count, cp, cj, cx);
    GRX_HIP_CHECK(hipGetLastError());
    ++launches;
  }
  if (int32_t r = p.rows_of(1)) {
    k::spgemm_group_kernel<k::SG_SMALL, NUMERIC>
        <<<grid_for((std::size_t)r, k::SG_BLOCK / k::SG_SMALL, p.sc), k::SG_BLOCK, 0, s>>>(
            o.ap, o.aj, o.ax, o.bp, o.bj, o.bx, p.rows_at(1), r, count, cp, cj, cx);
    GRX_HIP_CHECK(hipGetLastError());
    ++launches;
  }
  return launches;
}

}  // namespace

extern "C" int grx_spgemm(grx_context_t ctx, grx_graph_t a, grx_graph_t b, grx_graph_t* out, const grx_options* opt,
                          grx_stats* stats) {
  if (!ctx || !a || !b || !out)
    return invalid("grx_spgemm: NULL argument");
  if (a->n_cols != b->n_rows)
    return invalid("grx_spgemm: the shapes do not match (a.n_cols != b.n_rows)");
  if (opt && opt->max_iterations != 0)
    return invalid("grx_spgemm: max_iterations must be 0");
  const bool timed = opt && opt->collect_kernel_time;
  const int rc = guarded([&] {
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();
    const int32_t n = a->n_rows, n_cols = b->n_cols;
    if (stats)
      std::memset(stats, 0, sizeof *stats);

    // capacities: what a workgroup may hold of LDS, lowered by the test hook
    int32_t sym_slots = 0, num_slots = 0, sym_tile = 0, num_tile = 0;
    {
      int dev = 0, max_lds = 0;
      GRX_HIP_CHECK(hipGetDevice(&dev));
      GRX_HIP_CHECK(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
      const long long budget = (long long)max_lds - 1024;  // the static part stays below 1 KB
      const long long hook = env_or("GRX_SPGEMM_LDS_SLOTS", budget, k::SG_MIN_SLOTS, budget);
      sym_slots = pow2_floor(std::min(budget / 4, hook));  // 4 bytes per key
      num_slots = pow2_floor(std::min(budget / 8, hook));  // ... and 4 per value
      const long long cols32 = ((long long)n_cols + 31) / 32 * 32;
      // a tile's bytes: one bit per column, and 4 bytes more in the numeric phase
      sym_tile = (int32_t)std::max(32ll, std::min(cols32, std::min(budget, hook * 4) * 8));
      num_tile = (int32_t)std::max(32ll, std::min(cols32, std::min(budget, hook * 8) * 8 / 33 / 32 * 32));
    }
    const int32_t small_products =
        (int32_t)env_or("GRX_SPGEMM_SMALL_PRODUCTS", k::SG_SMALL_PRODUCTS, 0, k::SG_SMALL_PRODUCTS);

    auto c = std::make_unique<grx_graph_s>();
    c->n_rows = n;
    c->n_cols = n_cols;
    c->ap.resize((std::size_t)n + 1);

    call_clock_t clock(s, timed);
    clock.start();
    unsigned long long h_totals[3] = {0, 0, 0};  // products, entries of C, rows of C with an entry
    int32_t launches = 0;
    float phase_ms[3] = {0, 0, 0};
    bool too_large = false;
    if (n == 0) {
      GRX_HIP_CHECK(hipMemsetAsync(c->ap.data(), 0, sizeof(int32_t), s));
      c->aj.resize(1);
      c->ax.resize(1);
    } else {
      const operands_t o{a->d_ap, a->d_aj, a->d_ax, b->d_ap, b->d_aj, b->d_ax, n_cols};
      hip::device_array_t<unsigned long long> products((std::size_t)n), totals(3);
      hip::device_array_t<int32_t> bound((std::size_t)n), count((std::size_t)n);
      hip::device_array_t<unsigned char> temp(256);
      GRX_HIP_CHECK(hipMemsetAsync(totals.data(), 0, sizeof h_totals, s));
      GRX_HIP_CHECK(hipMemsetAsync(count.data(), 0, (std::size_t)n * sizeof(int32_t), s));  // empty rows stay 0
      const unsigned row_grid = grid_for((std::size_t)n, k::SG_BLOCK / hip::wave_size, sc);

      // 1. the products of every row
      clock.begin_batch();
      k::spgemm_bound_kernel<<<row_grid, k::SG_BLOCK, 0, s>>>(o.ap, o.aj, o.bp, n, n_cols, products.data(),
                                                              bound.data(), totals.data());
      GRX_HIP_CHECK(hipGetLastError());
      ++launches;
      clock.end_batch();

      // 2. symbolic: rows by their bound, distinct columns per row
      phase_t phase(sc, n, temp);
      drain_t drain{s};  // after the workspace above: nothing of it is released under a running kernel
      phase.bin(class_key_t{bound.data(), products.data(),
                            {std::min(k::SG_WAVE, sym_slots / 2), std::min(k::SG_MEDIUM, sym_slots / 2), sym_slots / 2},
                            small_products});
      if (timed)
        phase_ms[0] = clock.kernel_ms();
      clock.begin_batch();
      launches += launch_phase<false>(phase, o, bound.data(), sym_slots, sym_tile, count.data(), nullptr, nullptr,
                                      nullptr);
      k::spgemm_sum_kernel<<<grid_for((std::size_t)n, k::SG_BLOCK, sc), k::SG_BLOCK, 0, s>>>(count.data(), n,
                                                                                               totals.data());
      GRX_HIP_CHECK(hipGetLastError());
      ++launches;
      clock.end_batch();
      GRX_HIP_CHECK(hipMemcpyAsync(h_totals, totals.data(), sizeof h_totals, hipMemcpyDeviceToHost, s));
      GRX_HIP_CHECK(hipStreamSynchronize(s));
      if (timed)
        phase_ms[1] = clock.kernel_ms() - phase_ms[0];

      // 3. row offsets, and C itself unless it is more than a handle holds
      too_large = h_totals[1] > (unsigned long long)INT32_MAX;
      if (!too_large) {
        auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int32_t>(0),
                                                   padded_t{count.data(), n});
        const std::size_t bytes = hip::exclusive_sum_temp_bytes(in, c->ap.data(), int32_t(0), (std::size_t)n + 1);
        if (temp.size() < bytes)
          temp.resize(bytes);
        hip::exclusive_sum(temp.data(), bytes, in, c->ap.data(), int32_t(0), (std::size_t)n + 1, s);
        c->aj.resize((std::size_t)std::max<unsigned long long>(h_totals[1], 1));
        c->ax.resize((std::size_t)std::max<unsigned long long>(h_totals[1], 1));

        // 4. numeric: rows by their exact length
        phase.bin(class_key_t{count.data(), products.data(),
                              {std::min(k::SG_WAVE, num_slots / 2), std::min(k::SG_MEDIUM, num_slots / 2),
                               num_slots / 2},
                              small_products});
        clock.begin_batch();
        launches += launch_phase<true>(phase, o, count.data(), num_slots, num_tile, nullptr, c->ap.data(),
                                       c->aj.data(), c->ax.data());
        clock.end_batch();
      }
    }
    clock.stop_and_wait();
    if (timed)
      phase_ms[2] = clock.kernel_ms() - phase_ms[0] - phase_ms[1];
    if (too_large)
      return unsupported(("grx_spgemm: the product has " + std::to_string(h_totals[1]) +
                          " entries, more than the 2147483647 a handle holds")
                             .c_str());
    c->nnz = (int64_t)h_totals[1];
    c->adopt();
    *out = c.release();
    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->iterations = 1;
      stats->advance_launches = launches;
      stats->vertices_reached = (int64_t)h_totals[2];
      stats->edges_traversed = (int64_t)h_totals[1];
      stats->edges_expanded = (int64_t)h_totals[0];
      if (timed) {
        stats->levels_recorded = 3;
        for (int p = 0; p < 3; ++p)
          stats->frontier_slots[p] = (int64_t)(phase_ms[p] * 1000.0f + 0.5f);
      }
    }
    return (int)GRX_OK;
  });
  // the workspace is large and of no use to the operators: do not park it
  hip::block_cache_t::instance().trim();
  return rc;
}

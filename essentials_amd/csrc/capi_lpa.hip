/** @file capi_lpa.hip  grx_lpa: communities by semi-synchronous label propagation over the colour
 * classes of grx_color, and grx_modularity: the score of any labelling in exact integers
 * (hip/kernels/lpa_kernels.hxx).  No reference counterpart.  The vertices are sorted once by
 * (colour, row-length bin); a sweep is one launch per non-empty bin of every large class and one
 * one-workgroup launch per run of small classes, and ends with the one hand-off that carries the
 * sweep's change count. */
#include "capi_batch.hxx"

#include <gunrock/hip/kernels/lpa_kernels.hxx>

#include <cstring>

using namespace essentials_amd;

namespace {

namespace k = gunrock::hip::kernels;

/// Q from its integer parts, in exactly this form.
double modularity_of(unsigned long long inside, unsigned long long squares, int64_t entries) {
  if (entries == 0)
    return 0.0;
  return (double)inside / (double)entries - (double)squares / ((double)entries * (double)entries);
}

/// Enqueue the modularity passes over `label`: the range check, tot, I and S land in `ctr`.  `tot`:
/// V words, zeroed here; `big`: big_list_size(g) items.  Returns the launches.
int32_t enqueue_modularity(gcuda::standard_context_t& sc, grx_graph_s* g, const int32_t* label, unsigned* tot,
                           int2* big, k::lpa_counters_t* ctr) {
  const hipStream_t s = sc.stream();
  const int32_t n = g->n_rows;
  const unsigned grid = grid_for((std::size_t)n, k::LPA_BLOCK, sc);
  GRX_HIP_CHECK(hipMemsetAsync(tot, 0, sizeof(unsigned) * (std::size_t)n, s));
  k::lpa_range_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(label, n, ctr);
  k::lpa_tot_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(g->d_ap, label, n, tot);
  k::lpa_inside_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(g->d_ap, g->d_aj, label, n, big, ctr);
  k::lpa_inside_big_kernel<<<(unsigned)sc.compute_units() * 4, k::LPA_BLOCK, 0, s>>>(g->d_ap, g->d_aj, label, big, ctr);
  k::lpa_squares_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(tot, n, ctr);
  GRX_HIP_CHECK(hipGetLastError());
  return 5;
}

/// Items of the big list: a row above the segment length has at most d / segment + 1 segments.
std::size_t big_list_size(const grx_graph_s* g) {
  return 2 * ((std::size_t)g->nnz / k::LPA_INSIDE_SEGMENT) + 1;
}

/// Consecutive colour classes that one launch sequence serves: one wide class, or a run of small ones.
struct step_t {
  int32_t c0, c1;
  bool narrow;
};

}  // namespace

extern "C" int grx_modularity(grx_context_t ctx, grx_graph_t g, const int32_t* d_label, double* h_modularity,
                              int64_t* h_inside_entries, uint64_t* h_degree_squares, const grx_options* opt,
                              grx_stats* stats) {
  if (!ctx || !g || (!d_label && g->n_rows > 0))  // the labels of no vertices may be nowhere
    return invalid("grx_modularity: NULL argument");
  if (!h_modularity && !h_inside_entries && !h_degree_squares)
    return invalid("grx_modularity: all three outputs are NULL");
  if (g->n_rows != g->n_cols)
    return invalid("grx_modularity: the graph is not square (n_rows != n_cols)");
  const bool timed = opt && opt->collect_kernel_time;
  return guarded([&] {
    const int32_t n = g->n_rows;
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    unsigned long long inside = 0, squares = 0;
    int32_t launches = 0;
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();
    call_clock_t clock(s, timed);
    clock.start();
    if (n > 0) {
      hip::device_array_t<unsigned> tot((std::size_t)n);
      hip::device_array_t<int2> big(big_list_size(g));
      hip::device_array_t<k::lpa_counters_t> counters(1);
      k::lpa_counters_t* ctr = counters.data();
      GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof *ctr, s));
      clock.begin_batch();
      launches += enqueue_modularity(sc, g, d_label, tot.data(), big.data(), ctr);
      const unsigned long long* m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
        k::lpa_publish_kernel<<<1, 64, 0, s>>>(ctr, mirror, slot, seq);
      });
      ++launches;
      const bool bad = m[k::LPA_BAD] != 0;
      inside = m[k::LPA_INSIDE];
      squares = m[k::LPA_SQUARES];
      clock.stop_and_wait();
      if (bad)
        return invalid("grx_modularity: a label is outside [0, V)");
    } else {
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();
    if (h_modularity)
      *h_modularity = modularity_of(inside, squares, g->nnz);
    if (h_inside_entries)
      *h_inside_entries = (int64_t)inside;
    if (h_degree_squares)
      *h_degree_squares = (uint64_t)squares;
    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->iterations = 1;
      stats->advance_launches = launches;
      stats->edges_traversed = g->nnz;
      stats->edges_expanded = g->nnz;
    }
    return (int)GRX_OK;
  });
}

extern "C" int grx_lpa(grx_context_t ctx, grx_graph_t g, int32_t* d_community, int64_t* h_communities,
                       double* h_modularity, const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_lpa: NULL argument");
  if (!d_community && !h_communities && !h_modularity)
    return invalid("grx_lpa: all three outputs are NULL");
  if (g->n_rows != g->n_cols)
    return invalid("grx_lpa: the graph is not square (n_rows != n_cols)");
  if (opt && opt->max_iterations < 0)
    return invalid("grx_lpa: max_iterations must not be negative");
  const bool timed = opt && opt->collect_kernel_time;
  const int32_t max_sweeps = opt ? opt->max_iterations : 0;
  return guarded([&] {
    const int32_t n = g->n_rows;
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (h_communities)
      *h_communities = 0;
    if (h_modularity)
      *h_modularity = 0.0;
    if (n == 0)  // the empty graph: nothing to write
      return (int)GRX_OK;
    if (int rc = require_symmetric(ctx, g, "grx_lpa", "label propagation"))
      return rc;
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();

    // test hooks: the row length above which a row gets 1024 threads and the largest table, the
    // entries a class may have to run in the one-workgroup kernel (0 sends every class to the wide
    // kernels), whether every vertex decides every sweep, and the slots of the largest LDS table
    const int32_t big_row = (int32_t)env_or("GRX_LPA_BIG_ROW", k::LPA_BIG_ROW, 1, INT32_MAX);
    const unsigned long long narrow_edges =
        (unsigned long long)env_or("GRX_LPA_NARROW_EDGES", k::LPA_NARROW_EDGES, 0, 1ll << 30);
    const bool all_rows = env_flag("GRX_LPA_ALL_ROWS", false);
    int32_t slots = 0;
    {
      int dev = 0, max_lds = 0;
      GRX_HIP_CHECK(hipGetDevice(&dev));
      GRX_HIP_CHECK(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
      const long long most = ((long long)max_lds - 1024) / 8;  // a key and a count; the static part stays below 1 KB
      slots = (int32_t)env_or("GRX_LPA_LDS_SLOTS", most, k::LPA_MIN_SLOTS, most);
    }
    k::lpa_key_t key{nullptr, g->d_ap, {0, 0, 0}};
    key.b[0] = std::min(k::LPA_SMALL_ROW, big_row);
    key.b[1] = std::min(k::LPA_WAVE_ROW, big_row);
    key.b[2] = std::max(key.b[1], std::min(big_row, slots / 2));  // a medium row's table never overflows
    const int32_t medium_slots = (int32_t)k::lpa_slots_for(key.b[2], slots);

    call_clock_t clock(s, timed);
    clock.start();

    int32_t launches = 0, sweeps = 0;
    unsigned long long read = 0, communities = 0, inside = 0, squares = 0;
    std::vector<unsigned long long> changed;
    {
      // 1. the colour classes
      hip::device_array_t<int32_t> color((std::size_t)n);
      int32_t num_colors = 0;
      if (int rc = grx_color(ctx, g, color.data(), &num_colors, nullptr, nullptr))
        return rc;
      key.color = color.data();
      const int32_t n_keys = num_colors * k::LPA_BINS;
      int bits = 1;
      while ((1ll << bits) < n_keys)
        ++bits;

      // 2. the vertices by (class, bin), ascending ids within; sizes and entry totals to the host
      hip::device_array_t<unsigned> keys((std::size_t)n);
      hip::device_array_t<int32_t> order((std::size_t)n), starts((std::size_t)n_keys + 1);
      hip::device_array_t<unsigned long long> entries((std::size_t)n_keys);
      std::vector<int32_t> h_starts((std::size_t)n_keys + 1);
      std::vector<unsigned long long> h_entries((std::size_t)n_keys);
      clock.begin_batch();
      {
        auto key_it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int32_t>(0), key);
        std::size_t bytes = 0;
        GRX_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, key_it, keys.data(),
                                                rocprim::make_counting_iterator<int32_t>(0), order.data(), (std::size_t)n,
                                                0, bits, s));
        hip::device_array_t<unsigned char> temp(std::max<std::size_t>(bytes, 256));
        GRX_HIP_CHECK(rocprim::radix_sort_pairs(temp.data(), bytes, key_it, keys.data(),
                                                rocprim::make_counting_iterator<int32_t>(0), order.data(), (std::size_t)n,
                                                0, bits, s));
        GRX_HIP_CHECK(hipMemsetAsync(entries.data(), 0, sizeof(unsigned long long) * (std::size_t)n_keys, s));
        k::lpa_starts_kernel<<<grid_for((std::size_t)n_keys + 1, k::LPA_BLOCK, sc), k::LPA_BLOCK, 0, s>>>(
            keys.data(), n, n_keys, starts.data());
        k::lpa_entries_kernel<<<grid_for((std::size_t)n, k::LPA_BLOCK, sc), k::LPA_BLOCK, 0, s>>>(
            keys.data(), order.data(), g->d_ap, n, entries.data());
        GRX_HIP_CHECK(hipGetLastError());
        launches += 3;
        clock.end_batch();
        GRX_HIP_CHECK(hipMemcpyAsync(h_starts.data(), starts.data(), h_starts.size() * sizeof(int32_t),
                                     hipMemcpyDeviceToHost, s));
        GRX_HIP_CHECK(hipMemcpyAsync(h_entries.data(), entries.data(), h_entries.size() * sizeof(unsigned long long),
                                     hipMemcpyDeviceToHost, s));
        GRX_HIP_CHECK(hipStreamSynchronize(s));  // the sort's temporary storage is released behind it
      }

      // 3. the launch plan of a sweep, and what the overflow paths may need
      std::vector<step_t> steps;
      unsigned long long pool_entries = 0;
      std::size_t over_rows = 0;
      for (int32_t c = 0; c < num_colors; ++c) {
        const int32_t* at = h_starts.data() + k::LPA_BINS * c;
        const unsigned long long* e = h_entries.data() + k::LPA_BINS * c;
        const int32_t size = at[k::LPA_BINS] - at[0];
        if (size == 0)
          continue;
        const bool narrow =
            narrow_edges && size <= k::LPA_NARROW_VERTICES && e[0] + e[1] + e[2] + e[3] <= narrow_edges;
        if (narrow) {
          pool_entries = std::max(pool_entries, e[2] + e[3]);  // at least its longest row
          if (!steps.empty() && steps.back().narrow && steps.back().c1 == c)
            steps.back().c1 = c + 1;
          else
            steps.push_back({c, c + 1, true});
        } else {
          pool_entries = std::max(pool_entries, e[3]);
          over_rows = std::max<std::size_t>(over_rows, (std::size_t)(at[4] - at[3]));
          steps.push_back({c, c + 1, false});
        }
      }
      error::throw_if_exception(pool_entries > (unsigned long long)INT32_MAX, "grx_lpa: more entries than a CSR holds");

      hip::device_array_t<int32_t> own_label(d_community ? 0 : (std::size_t)n);
      hip::device_array_t<unsigned char> dirty(all_rows ? 0 : (std::size_t)n);
      hip::device_array_t<int32_t> pool(4 * (std::size_t)pool_entries + 4);
      hip::device_array_t<unsigned long long> over(over_rows + 1);
      hip::device_array_t<unsigned> tot(h_modularity ? (std::size_t)n : 0);
      hip::device_array_t<int2> big(h_modularity ? big_list_size(g) : 0);
      hip::device_array_t<k::lpa_counters_t> counters(1);
      k::lpa_counters_t* ctr = counters.data();
      int32_t* label = d_community ? d_community : own_label.data();
      const k::lpa_state_t st{g->d_ap, g->d_aj, label, all_rows ? nullptr : dirty.data()};

      const std::size_t medium_lds = 2 * sizeof(int32_t) * (std::size_t)medium_slots;
      const std::size_t big_lds = 2 * sizeof(int32_t) * (std::size_t)slots;
      const std::size_t narrow_lds =
          std::max(big_lds, 2 * sizeof(int32_t) * (std::size_t)k::LPA_WAVE_SLOTS * (k::LPA_BIG_BLOCK / hip::wave_size));
      GRX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k::lpa_block_kernel<k::LPA_BLOCK>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)medium_lds));
      GRX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k::lpa_block_kernel<k::LPA_BIG_BLOCK>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)big_lds));
      GRX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k::lpa_narrow_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)narrow_lds));

      auto wide = [&](int32_t c) {
        const int32_t* at = h_starts.data() + k::LPA_BINS * c;
        const int32_t* rows = order.data();
        if (const int32_t r = at[1] - at[0]) {
          k::lpa_group_kernel<k::LPA_SMALL>
              <<<grid_for((std::size_t)r, k::LPA_BLOCK / k::LPA_SMALL, sc), k::LPA_BLOCK, 0, s>>>(st, rows + at[0], r, ctr);
          ++launches;
        }
        if (const int32_t r = at[2] - at[1]) {
          k::lpa_group_kernel<hip::wave_size>
              <<<grid_for((std::size_t)r, k::LPA_BLOCK / hip::wave_size, sc), k::LPA_BLOCK, 0, s>>>(st, rows + at[1], r,
                                                                                                   ctr);
          ++launches;
        }
        if (const int32_t r = at[3] - at[2]) {
          k::lpa_block_kernel<k::LPA_BLOCK><<<grid_for((std::size_t)r, 1, sc), k::LPA_BLOCK, medium_lds, s>>>(
              st, rows + at[2], r, medium_slots, over.data(), ctr);
          ++launches;
        }
        if (const int32_t r = at[4] - at[3]) {
          // the class's overflow list and its share of the pool start empty
          GRX_HIP_CHECK(hipMemsetAsync(&ctr->overflow_n, 0, 2 * sizeof(int), s));
          k::lpa_block_kernel<k::LPA_BIG_BLOCK><<<grid_for((std::size_t)r, 1, sc), k::LPA_BIG_BLOCK, big_lds, s>>>(
              st, rows + at[3], r, slots, over.data(), ctr);
          k::lpa_fallback_kernel<<<std::min<unsigned>((unsigned)r, (unsigned)sc.compute_units()), k::LPA_BIG_BLOCK, 0,
                                   s>>>(st, over.data(), pool.data(), ctr);
          launches += 2;
        }
      };

      // 4. sweeps until one changes nothing
      GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof *ctr, s));
      clock.begin_batch();
      k::lpa_init_kernel<<<grid_for((std::size_t)n, k::LPA_BLOCK, sc), k::LPA_BLOCK, 0, s>>>(label, st.dirty, n);
      ++launches;
      const unsigned long long* m = nullptr;
      for (;;) {
        // every changing sweep raises the entries whose ends share a label by at least 2, and there
        // are nnz of them: more sweeps is a fault of the kernels, not a spin
        error::throw_if_exception((long long)sweeps >= (long long)g->nnz / 2 + 2,
                                  "grx_lpa: more sweeps than the entries allow");
        for (const step_t& step : steps) {
          if (step.narrow) {
            k::lpa_narrow_kernel<<<1, k::LPA_BIG_BLOCK, narrow_lds, s>>>(st, order.data(), starts.data(), step.c0,
                                                                        step.c1, slots, pool.data(), ctr);
            ++launches;
          } else {
            wide(step.c0);
          }
        }
        m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
          k::lpa_publish_kernel<<<1, 64, 0, s>>>(ctr, mirror, slot, seq);
        });
        ++launches;
        ++sweeps;
        changed.push_back(m[k::LPA_CHANGES]);
        read = m[k::LPA_READ];
        if (changed.back() == 0 || sweeps == max_sweeps)
          break;
        clock.begin_batch();
      }

      // 5. the smallest member names its community; the score of the result
      unsigned* first = keys.data();  // the sorted keys are done with
      clock.begin_batch();
      GRX_HIP_CHECK(hipMemsetAsync(first, 0xff, sizeof(unsigned) * (std::size_t)n, s));
      const unsigned grid = grid_for((std::size_t)n, k::LPA_BLOCK, sc);
      k::lpa_first_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(label, n, first);
      k::lpa_canonical_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(label, n, first, ctr);
      launches += 2;
      if (h_modularity)
        launches += enqueue_modularity(sc, g, label, tot.data(), big.data(), ctr);
      m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
        k::lpa_publish_kernel<<<1, 64, 0, s>>>(ctr, mirror, slot, seq);
      });
      ++launches;
      communities = m[k::LPA_COMMUNITIES];
      inside = m[k::LPA_INSIDE];
      squares = m[k::LPA_SQUARES];
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();

    if (h_communities)
      *h_communities = (int64_t)communities;
    if (h_modularity)
      *h_modularity = modularity_of(inside, squares, g->nnz);
    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->iterations = sweeps;
      stats->advance_launches = launches;
      stats->vertices_reached = (int64_t)n - (int64_t)communities;
      stats->edges_traversed = g->nnz;
      stats->edges_expanded = (int64_t)read;
      stats->levels_recorded = std::min(sweeps, 64);
      for (int32_t t = 0; t < stats->levels_recorded; ++t)
        stats->frontier_slots[t] = (int64_t)changed[(std::size_t)t];
    }
    return (int)GRX_OK;
  });
}

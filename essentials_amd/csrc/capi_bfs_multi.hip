/** @file capi_bfs_multi.hip  grx_bfs_multi: depths from many sources, 64 searches to a 64-bit word
 * per vertex (hip/kernels/bfs_multi_kernels.hxx).  No reference counterpart.  A batch is a seed, then
 * per level the expanding kernels (push over the active list, or pull over every unfinished vertex),
 * the update pass and the publish kernel: one hand-off per level. */
#include "capi_batch.hxx"

#include <gunrock/hip/kernels/bfs_multi_kernels.hxx>

using namespace essentials_amd;

namespace k = gunrock::hip::kernels;

extern "C" int grx_bfs_multi(grx_context_t ctx, grx_graph_t g, const int32_t* h_sources, int32_t n_sources,
                             int32_t* d_depths, int64_t* h_reached, int64_t* h_depth_sum, int32_t* h_eccentricity,
                             const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g)
    return invalid("grx_bfs_multi: NULL argument");
  if (n_sources < 0)
    return invalid("grx_bfs_multi: n_sources < 0");
  if (!h_sources && n_sources != 0)
    return invalid("grx_bfs_multi: h_sources is NULL (every vertex) but n_sources != 0");
  for (int32_t i = 0; i < n_sources; ++i)
    if (h_sources[i] < 0 || h_sources[i] >= g->n_rows)
      return invalid("grx_bfs_multi: source out of range");
  if (!d_depths && !h_reached && !h_depth_sum && !h_eccentricity)
    return invalid("grx_bfs_multi: all four outputs are NULL");
  if (g->n_rows != g->n_cols)
    return invalid("grx_bfs_multi: the graph is not square (n_rows != n_cols)");
  const grx_options o = effective_options(opt);
  if (o.max_iterations != 0)
    return invalid("grx_bfs_multi: max_iterations must be 0 (a truncated search has no summaries)");
  const bool timed = o.collect_kernel_time != 0;
  const bool may_pull = o.direction_optimized != 0;
  const double alpha = o.do_alpha > 0 ? (double)o.do_alpha : 4.0;
  return guarded([&] {
    const int32_t n = g->n_rows;
    const int64_t count = h_sources ? (int64_t)n_sources : (int64_t)n;
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (n == 0 || count == 0)  // nothing to search: nothing is written, nothing is launched
      return (int)GRX_OK;
    if (may_pull)
      if (int rc = ensure_can_pull(ctx, g)) {  // grx_bfs's status; the message names this call
        last_error() = "grx_bfs_multi: " + last_error();
        return rc;
      }
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();

    // test hook: the row length above which a row goes to whole workgroups
    const int32_t big_row = (int32_t)env_or("GRX_BFSM_BIG_ROW", k::BFSM_BIG_ROW, 1, INT32_MAX);

    call_clock_t clock(s, timed);
    clock.start();

    long long levels_total = 0, pulls = 0, launches = 0;
    unsigned long long reached_total = 0, traversed = 0, expanded = 0, pull_read = 0;
    {
      const std::size_t nv = (std::size_t)n, nnz = (std::size_t)g->nnz;
      // 32 bytes per vertex: seen and the two frontier arrays (8 each), the two lists (4 each)
      hip::device_array_t<k::bfsm_word_t> words(3 * nv);
      hip::device_array_t<int32_t> lists(2 * nv);
      hip::device_array_t<int2> big_segments(nnz / k::BFSM_BIG_SEGMENT + nnz / big_row + 1);
      hip::device_array_t<int32_t> big_rows(may_pull ? nnz / big_row + 1 : 0);
      hip::device_array_t<k::bfsm_counters_t> counters(1);
      k::bfsm_counters_t* ctr = counters.data();
      k::bfsm_word_t* seen = words.data();
      const k::bfsm_rows_t out{g->d_ap, g->d_aj};
      const k::bfsm_rows_t in =
          g->in_edges ? k::bfsm_rows_t{g->in_edges->offsets.data(), g->in_edges->indices.data()} : out;
      const unsigned most = (unsigned)sc.compute_units() * 8, settlers = (unsigned)sc.compute_units() * 4;
      k::bfsm_counters_t h_ctr;

      for (int64_t first = 0; first < count; first += k::BFSM_BATCH) {
        const int bits = (int)std::min<int64_t>(k::BFSM_BATCH, count - first);
        const k::bfsm_word_t mask = bits == k::BFSM_BATCH ? ~0ull : (1ull << bits) - 1;
        k::bfsm_sources_t src{};
        for (int i = 0; i < bits; ++i)
          src.v[i] = h_sources ? h_sources[first + i] : (int32_t)(first + i);
        int32_t* depth = d_depths ? d_depths + (std::size_t)first * nv : nullptr;

        clock.begin_batch();
        GRX_HIP_CHECK(hipMemsetAsync(words.data(), 0, 3 * nv * sizeof(k::bfsm_word_t), s));
        GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof *ctr, s));
        if (depth)
          GRX_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)depth, INT32_MAX, (std::size_t)bits * nv, s));
        k::bfsm_word_t* front = words.data() + nv;       // level L: empty until the seeds are settled
        k::bfsm_word_t* next = words.data() + 2 * nv;    // level L + 1
        int32_t* active = lists.data();
        int32_t* list = lists.data() + nv;
        auto output = [&](int32_t level) { return k::bfsm_out_t{seen, next, depth, list, out.ap, n, level, ctr}; };
        // settle what `next` and `list` hold as `level`, clear the words of the list it came from,
        // hand the new list's facts over and make it the active one
        unsigned long long* m = nullptr;
        auto finish_level = [&](int32_t level, bool settle, std::size_t at_most, int32_t old_count) {
          k::bfsm_update_kernel<<<hip::grid_for(std::max(at_most, (std::size_t)old_count), k::BFSM_BLOCK, settlers),
                                  k::BFSM_BLOCK, 0, s>>>(output(level), settle ? 1 : 0, front, active, old_count);
          m = hand_off(sc, clock, [&](unsigned long long* mirror, int slot, unsigned long long seq) {
            k::bfsm_publish_kernel<<<1, k::BFSM_BATCH, 0, s>>>(ctr, level, mirror, slot, seq);
          });
          launches += 2;
          std::swap(front, next);
          std::swap(active, list);
        };

        k::bfsm_seed_kernel<<<1, k::BFSM_BATCH, 0, s>>>(src, bits, next, list, n, ctr);
        ++launches;
        finish_level(0, true, (std::size_t)bits, 0);

        int32_t level = 0;  // of the active list
        for (;;) {
          const int32_t active_n = (int32_t)std::min<unsigned long long>(m[k::BM_TAIL], (unsigned long long)n);
          const unsigned long long degsum = m[k::BM_DEGSUM];
          if (active_n == 0)
            break;
          if (first == 0 && level < 64 && stats) {
            stats->frontier_slots[level] = active_n;
            stats->levels_recorded = level + 1;
          }
          ++levels_total;
          traversed += degsum;
          if (degsum == 0)  // no row to expand: the level after this one is empty
            break;
          // every level adds a depth, and a vertex has one per search: more than V levels is a fault
          error::throw_if_exception(level >= n, "grx_bfs_multi: more levels than vertices");
          clock.begin_batch();
          if (may_pull && (double)degsum * alpha > (double)g->nnz) {
            k::bfsm_pull_kernel<<<grid_for(nv, k::BFSM_BLOCK, sc), k::BFSM_BLOCK, 0, s>>>(in, front, output(level + 1),
                                                                                         mask, big_row, big_rows.data());
            k::bfsm_pull_big_kernel<<<most, k::BFSM_BLOCK, 0, s>>>(in, front, output(level + 1), mask, big_rows.data());
            launches += 2;
            ++pulls;
            finish_level(level + 1, false, 0, active_n);
          } else {
            const int32_t chunk =
                std::max<int32_t>(1, std::min<int32_t>(k::BFSM_BLOCK, (int32_t)((active_n + most - 1) / most)));
            k::bfsm_push_kernel<<<grid_for((std::size_t)active_n, (std::size_t)chunk, sc), k::BFSM_BLOCK, 0, s>>>(
                out, active, active_n, chunk, front, seen, next, list, n, big_row, big_segments.data(), ctr);
            ++launches;
            if (m[k::BM_MAX_ROW] > (unsigned long long)big_row) {
              k::bfsm_push_big_kernel<<<most, k::BFSM_BLOCK, 0, s>>>(out, front, seen, next, list, n, big_segments.data(),
                                                                    ctr);
              ++launches;
            }
            expanded += degsum;
            // an entry appends at most one vertex
            finish_level(level + 1, true, (std::size_t)std::min<unsigned long long>(degsum, nv), active_n);
          }
          ++level;
        }
        pull_read = m[k::BM_READ];

        // the batch's totals: every kernel that wrote them is behind the last hand-off
        GRX_HIP_CHECK(hipMemcpyAsync(&h_ctr, ctr, sizeof h_ctr, hipMemcpyDeviceToHost, s));
        GRX_HIP_CHECK(hipStreamSynchronize(s));
        for (int i = 0; i < bits; ++i) {
          if (h_reached)
            h_reached[first + i] = (int64_t)h_ctr.reached[i];
          if (h_depth_sum)
            h_depth_sum[first + i] = (int64_t)h_ctr.depth_sum[i];
          if (h_eccentricity)
            h_eccentricity[first + i] = h_ctr.eccentricity[i];
          reached_total += h_ctr.reached[i];
        }
        expanded += pull_read;  // counted on the device, from 0 with every batch
      }
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();

    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->iterations = (int32_t)std::min<long long>(levels_total, INT32_MAX);
      stats->advance_launches = (int32_t)std::min<long long>(launches, INT32_MAX);
      stats->pull_iterations = (int32_t)std::min<long long>(pulls, INT32_MAX);
      stats->vertices_reached = (int64_t)reached_total;
      stats->edges_traversed = (int64_t)traversed;
      stats->edges_expanded = (int64_t)expanded;
    }
    return (int)GRX_OK;
  });
}

/** @file capi_bc.hip  grx_bc == gunrock::bc::run summed over a list of sources (reference
 * algorithms/bc.hxx), deterministic: the sweeps pull (hip/kernels/bc_kernels.hxx). */
#include "capi_batch.hxx"
#include "capi_traversal.hxx"

#include <gunrock/hip/kernels/bc_kernels.hxx>

using namespace essentials_amd;

namespace {

namespace k = gunrock::hip::kernels;

/// Sort key of a vertex: its depth, `cap` when unreached (depths stay below cap).
struct depth_key_t {
  const int32_t* depth;
  unsigned cap;
  __host__ __device__ unsigned operator()(int32_t v) const {
    const int32_t d = depth[v];
    return (unsigned)d < cap ? (unsigned)d : cap;
  }
};

/// Chunk slots of position p of the level list (0 past the reached vertices and at p == n).
struct chunk_count_t {
  const unsigned* keys;
  const int32_t* verts;
  const int32_t* ap;
  const int32_t* in_ap;
  int32_t n;
  unsigned cap;
  __host__ __device__ int32_t operator()(int32_t p) const {
    if (p >= n || keys[p] >= cap)
      return 0;
    const int32_t v = verts[p];
    return k::bc_chunks_of(in_ap[v + 1] - in_ap[v], ap[v + 1] - ap[v]);
  }
};

}  // namespace

extern "C" int grx_bc(grx_context_t ctx, grx_graph_t g, const int32_t* h_sources, int32_t n_sources,
                      float* d_bc, const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g || !d_bc)
    return invalid("grx_bc: NULL argument");
  if (n_sources < 0)
    return invalid("grx_bc: n_sources < 0");
  if (!h_sources && n_sources != 0)
    return invalid("grx_bc: h_sources is NULL (every vertex) but n_sources != 0");
  for (int32_t i = 0; i < n_sources; ++i)
    if (h_sources[i] < 0 || h_sources[i] >= g->n_rows)
      return invalid("grx_bc: source out of range");
  grx_options o = effective_options(opt);
  if (o.max_iterations != 0)
    return invalid("grx_bc: max_iterations must be 0 (a truncated search gives wrong centralities)");
  return guarded([&] {
    return with_load_balance(o.load_balance, [&](auto lb_tag) -> int {
      constexpr auto lb = decltype(lb_tag)::value;
      using problem_type = clients::bfs_problem_t<graph_type>;
      // the forward sweep walks in-edges
      if (int rc = ensure_can_pull(ctx, g))
        return rc;
      auto& sc = ctx->single();
      const hipStream_t s = sc.stream();
      scoped_options scope(sc, &o);
      // depths, sweeps and sums run on the hot-first copy when grx_bfs would (a directed graph
      // with attached in-edges keeps the caller's numbering: hot_copy says no); bc is delivered
      // in the caller's numbering once, at the end
      const run_graph_t run = run_graph(ctx, g, !o.call_every_edge && !o.holes_layout);
      const bool renumbered = run.renumbered();
      graph_type G = run.on->view();
      const auto in = G.in_edges();
      const int32_t* ap = run.on->d_ap;
      const int32_t* aj = run.on->d_aj;
      const int32_t* in_ap = in.get_row_offsets();
      const int32_t* in_aj = in.get_column_indices();
      const int32_t n = g->n_rows;
      const int32_t count = h_sources ? n_sources : n;
      if (stats)
        std::memset(stats, 0, sizeof *stats);

      // workspace of the call, reused by every source
      hip::device_array_t<int32_t> depth(n), verts(n), chunk_start((std::size_t)n + 1);
      hip::device_array_t<float> sigma(n), rho(n), work_bc(renumbered ? n : 0);
      unsigned* keys = reinterpret_cast<unsigned*>(rho.data());  // rho is written by the sweeps only
      hip::device_array_t<int32_t> bounds(2 * ((std::size_t)n + 2));  // level offsets, chunk offsets
      hip::device_array_t<unsigned long long> counters(2);
      // chunk slots: a hub row of max(in, out) degree m >= BC_HUB takes ceil(m / BC_CHUNK) <=
      // (in + out) / BC_CHUNK + 1 of them, and there are at most 2 nnz / BC_HUB hubs
      const std::size_t max_chunks = 2 * (std::size_t)g->nnz / k::BC_CHUNK + 2 * (std::size_t)g->nnz / k::BC_HUB + 1;
      hip::device_array_t<float> partial(max_chunks);
      hip::device_array_t<int32_t> owner(max_chunks);
      float* bc = renumbered ? work_bc.data() : d_bc;

      call_clock_t clock(s, false);
      clock.start();
      if (n)
        GRX_HIP_CHECK(hipMemsetAsync(bc, 0, (std::size_t)n * sizeof(float), s));

      // rocPRIM temporaries, sized once for the largest key range
      std::size_t sort_bytes = 0, scan_bytes = 0;
      {
        const unsigned all_bits = 32;
        auto key_it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int32_t>(0),
                                                       depth_key_t{depth.data(), (unsigned)n + 1});
        GRX_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, key_it, keys,
                                                rocprim::make_counting_iterator<int32_t>(0), verts.data(),
                                                (std::size_t)n, 0, all_bits, s));
        auto chunk_it = rocprim::make_transform_iterator(
            rocprim::make_counting_iterator<int32_t>(0),
            chunk_count_t{keys, verts.data(), ap, in_ap, n, (unsigned)n + 1});
        GRX_HIP_CHECK(rocprim::exclusive_scan(nullptr, scan_bytes, chunk_it, chunk_start.data(), int32_t(0),
                                              (std::size_t)n + 1, rocprim::plus<int32_t>(), s));
      }
      hip::device_array_t<unsigned char> temp(std::max<std::size_t>(256, std::max(sort_bytes, scan_bytes)));

      std::vector<int32_t> h_bounds;
      unsigned long long h_counters[2];
      long long levels_total = 0, reached_total = 0, edges_total = 0;

      for (int32_t i = 0; i < count; ++i) {
        const int32_t source = h_sources ? h_sources[i] : i;
        // 1. depths: the BFS client, in the numbering it runs in (max_iterations is 0: checked above)
        problem_type problem(G, run.vertex(source), depth.data(), ctx->mc);
        const int iterations = run_bfs_client<lb>(problem, n, o, ctx).iterations;
        levels_total += iterations;

        // 2. level lists: reached vertices stably sorted by depth (on the hot-first copy each
        // level then starts with its highest-degree vertices), level and chunk offsets
        const unsigned cap = (unsigned)iterations + 1;  // > every depth; the key of the unreached
        error::throw_if_exception((std::size_t)cap > (std::size_t)n + 1, "grx_bc: more levels than vertices");
        unsigned bits = 1;
        while (bits < 32 && (cap >> bits))
          ++bits;
        auto key_it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int32_t>(0),
                                                       depth_key_t{depth.data(), cap});
        std::size_t bytes = temp.size();
        GRX_HIP_CHECK(rocprim::radix_sort_pairs(temp.data(), bytes, key_it, keys,
                                                rocprim::make_counting_iterator<int32_t>(0), verts.data(),
                                                (std::size_t)n, 0, bits, s));
        int32_t* level_at = bounds.data();          // [0, cap]
        int32_t* chunk_at = bounds.data() + cap + 1;  // [0, cap]
        GRX_HIP_CHECK(hipMemsetAsync(counters.data(), 0, 2 * sizeof(unsigned long long), s));
        k::bc_level_bounds_kernel<<<grid_for((std::size_t)n, k::BC_BLOCK, sc), k::BC_BLOCK, 0, s>>>(
            keys, verts.data(), ap, n, cap, level_at, counters.data());
        GRX_HIP_CHECK(hipGetLastError());
        auto chunk_it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int32_t>(0),
                                                         chunk_count_t{keys, verts.data(), ap, in_ap, n, cap});
        bytes = temp.size();
        GRX_HIP_CHECK(rocprim::exclusive_scan(temp.data(), bytes, chunk_it, chunk_start.data(), int32_t(0),
                                              (std::size_t)n + 1, rocprim::plus<int32_t>(), s));
        k::bc_chunk_owner_kernel<<<grid_for((std::size_t)n, k::BC_BLOCK, sc), k::BC_BLOCK, 0, s>>>(
            chunk_start.data(), n, owner.data());
        GRX_HIP_CHECK(hipGetLastError());
        k::bc_hub_bounds_kernel<<<grid_for((std::size_t)cap + 1, k::BC_BLOCK, sc), k::BC_BLOCK, 0, s>>>(
            level_at, chunk_start.data(), cap, chunk_at);
        GRX_HIP_CHECK(hipGetLastError());
        // the only host wait of the source: its level and chunk offsets
        h_bounds.resize(2 * ((std::size_t)cap + 1));
        GRX_HIP_CHECK(hipMemcpyAsync(h_bounds.data(), bounds.data(), h_bounds.size() * sizeof(int32_t),
                                     hipMemcpyDeviceToHost, s));
        GRX_HIP_CHECK(hipMemcpyAsync(h_counters, counters.data(), sizeof h_counters, hipMemcpyDeviceToHost, s));
        GRX_HIP_CHECK(hipStreamSynchronize(s));
        const int32_t* lv = h_bounds.data();
        const int32_t* hb = h_bounds.data() + cap + 1;
        error::throw_if_exception((long long)h_counters[0] != (long long)lv[cap],
                                  "grx_bc: a reached vertex's depth exceeds the search's level count");
        reached_total += (long long)h_counters[0];
        edges_total += (long long)h_counters[1];
        int32_t D = 0;  // levels 0 .. D-1 are not empty
        while ((unsigned)D < cap && lv[D + 1] > lv[D])
          ++D;

        // 3. + 4. both sweeps, enqueued back to back: every size is known now
        auto level = [&](auto forward_tag, int32_t d) {
          constexpr bool FORWARD = decltype(forward_tag)::value;
          const int32_t* row_ap = FORWARD ? in_ap : ap;
          const int32_t* row_aj = FORWARD ? in_aj : aj;
          const int32_t want = FORWARD ? d - 1 : d + 1;
          const float* val = FORWARD ? sigma.data() : rho.data();
          const int32_t p_lo = lv[d], p_hi = lv[d + 1];
          const int32_t c_lo = hb[d], n_chunks = hb[d + 1] - hb[d];
          if (n_chunks > 0) {
            k::bc_hub_chunk_kernel<FORWARD><<<grid_for((std::size_t)n_chunks, 1, sc), k::BC_BLOCK, 0, s>>>(
                row_ap, row_aj, verts.data(), chunk_start.data(), owner.data(), c_lo, n_chunks, depth.data(), want,
                val, partial.data());
            GRX_HIP_CHECK(hipGetLastError());
          }
          k::bc_level_kernel<FORWARD>
              <<<grid_for((std::size_t)(p_hi - p_lo), k::BC_BLOCK / k::BC_GROUP, sc), k::BC_BLOCK, 0, s>>>(
                  row_ap, row_aj, verts.data(), chunk_start.data(), partial.data(), p_lo, p_hi - p_lo,
                  depth.data(), want, val, sigma.data(), rho.data(), bc);
          GRX_HIP_CHECK(hipGetLastError());
        };
        for (int32_t d = 1; d < D; ++d)
          level(std::true_type(), d);
        for (int32_t d = D - 2; d >= 1; --d)  // level D-1: delta = 0; level 0: the source
          level(std::false_type(), d);
      }

      // 5. the caller's numbering, once
      if (renumbered && n) {
        const float* from = work_bc.data();
        const int32_t* rank_of = g->hot_rank_of_device.data();
        float* out = d_bc;
        hip::for_each_index((std::size_t)n, [from, rank_of, out] __device__(std::size_t v) { out[v] = from[rank_of[v]]; },
                            s);
      }
      clock.stop_and_wait();
      if (stats) {
        stats->elapsed_ms = clock.elapsed_ms();
        stats->iterations = (int32_t)std::min<long long>(levels_total, INT32_MAX);
        stats->vertices_reached = reached_total;
        stats->edges_traversed = edges_total;
      }
      return (int)GRX_OK;
    });
  });
}

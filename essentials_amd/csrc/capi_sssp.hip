/** @file capi_sssp.hip  grx_sssp == gunrock::sssp::run (reference algorithms/sssp.hxx:155-185). */
#include "capi_traversal.hxx"

#include <rocprim/rocprim.hpp>

using namespace essentials_amd;

namespace essentials_amd {
/// Largest |V| for which grx_sssp keeps packed 64-bit labels (GRX_SSSP_PACKED_MAX_VERTICES overrides).
inline long long packed_sssp_max_vertices() {
  // 32 MB of labels: what the eight 4 MB L2s hold between them
  return env_or("GRX_SSSP_PACKED_MAX_VERTICES", 1ll << 22, LLONG_MIN, LLONG_MAX);
}

namespace {
/// key[e] = row(e) << 32 | order-preserving bits of weight(e): one global sort puts every row's
/// entries in ascending weight (ties: any order the sort leaves) under the graph's own offsets.
__global__ void __launch_bounds__(256)
    light_keys_kernel(const int32_t* ap, const float* ax, int32_t n_rows, long long nnz, unsigned long long* keys) {
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < nnz; e += (long long)gridDim.x * 256) {
    int32_t lo = 0, hi = n_rows;  // the last row r with ap[r] <= e: the one e lies in (empty rows before it lose)
    while (hi - lo > 1) {
      const int32_t mid = lo + (hi - lo) / 2;
      if ((long long)ap[mid] <= e)
        lo = mid;
      else
        hi = mid;
    }
    unsigned b;
    const float w = ax[e];
    memcpy(&b, &w, 4);
    b ^= (b >> 31) ? 0xffffffffu : 0x80000000u;
    keys[e] = ((unsigned long long)(unsigned)lo << 32) | b;
  }
}
/// record[e] = {neighbour, weight} as one 64-bit word: the neighbour in the low half.
__global__ void __launch_bounds__(256)
    light_records_kernel(const unsigned long long* keys, const int32_t* cols, long long nnz,
                         unsigned long long* records) {
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < nnz; e += (long long)gridDim.x * 256) {
    const unsigned u = (unsigned)keys[e];
    const unsigned b = u ^ ((u >> 31) ? 0x80000000u : 0xffffffffu);
    records[e] = ((unsigned long long)b << 32) | (unsigned)cols[e];
  }
}
__global__ void __launch_bounds__(256)
    lightest_kernel(const int32_t* ap, const unsigned long long* records, int32_t n_rows, float* lightest) {
  for (long long v = blockIdx.x * 256ll + threadIdx.x; v < n_rows; v += (long long)gridDim.x * 256) {
    float w = std::numeric_limits<float>::infinity();  // a row without entries is never opened
    if (ap[v + 1] > ap[v]) {
      const unsigned b = (unsigned)(records[ap[v]] >> 32);
      memcpy(&w, &b, 4);
    }
    lightest[v] = w;
  }
}
}  // namespace

const grx_graph_s::light_rows_s* light_rows(grx_context_s* ctx, grx_graph_s* g) {
  std::lock_guard<std::mutex> lock(g->hot_mutex);
  if (!g->weight_symmetric || g->in_edges || g->symmetry != grx_graph_s::symmetric || g->nnz < 1) {
    g->light.release();  // in-edges attached since: the handle says "directed" now, the rows are of no use
    return nullptr;
  }
  auto& L = g->light;
  if (L.ready)
    return &L;
  if (L.refused)
    return nullptr;
  auto& c = ctx->single();
  hipStream_t s = c.stream();
  const std::size_t nnz = (std::size_t)g->nnz;
  // Everything below may throw (an allocation that fails, any HIP error).  The handle is touched
  // only once the build is complete: until then it holds no arrays, the call that asked pushes as
  // it did before there was anything to pull, and a later call tries again.
  try {
    const float* ax = g->d_ax;
    const unsigned long long nans = hip::transform_reduce(
        nnz, [ax] __device__(std::size_t e) -> unsigned long long { return ax[e] != ax[e] ? 1ull : 0ull; }, 0ull,
        rocprim::plus<unsigned long long>(), c);
    if (nans) {  // no order to sort by: this graph pushes
      L.refused = true;
      return nullptr;
    }
    util::timer_t timer(s);
    timer.begin();
    hip::device_array_t<unsigned long long> records;
    hip::device_array_t<float> lightest;
    records.set_parking(false);
    lightest.set_parking(false);
    records.resize(nnz);
    lightest.resize((std::size_t)g->n_rows);
    // a test hook: fail where a failure is worst, with the arrays allocated and nothing in them
    error::throw_if_exception(env_flag("GRX_SSSP_PULL_BUILD_FAILS", false), "sssp pull rows: build made to fail");
    float ms = 0;
    {
      hip::buffer_t<unsigned long long> keys(nnz), keys2(nnz);
      hip::buffer_t<int32_t> cols2(nnz);
      const unsigned grid = (unsigned)c.compute_units() * 8;
      light_keys_kernel<<<grid, 256, 0, s>>>(g->d_ap, g->d_ax, g->n_rows, (long long)nnz, keys.data());
      GRX_HIP_CHECK(hipGetLastError());
      unsigned row_bits = 1;
      while (row_bits < 32 && (1ull << row_bits) < (unsigned long long)g->n_rows)
        ++row_bits;
      std::size_t bytes = 0;
      GRX_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, keys.data(), keys2.data(), g->d_aj, cols2.data(), nnz,
                                              0, 32 + row_bits, s));
      hip::buffer_t<unsigned char> temp(bytes < 256 ? 256 : bytes);  // never null: rocPRIM would only size
      GRX_HIP_CHECK(rocprim::radix_sort_pairs(temp.data(), bytes, keys.data(), keys2.data(), g->d_aj, cols2.data(),
                                              nnz, 0, 32 + row_bits, s));
      light_records_kernel<<<grid, 256, 0, s>>>(keys2.data(), cols2.data(), (long long)nnz, records.data());
      lightest_kernel<<<grid, 256, 0, s>>>(g->d_ap, records.data(), g->n_rows, lightest.data());
      GRX_HIP_CHECK(hipGetLastError());
      ms = timer.end();  // synchronises: the arrays are complete, the sort's buffers may go
    }
    L.records = std::move(records);
    L.lightest = std::move(lightest);
    L.build_ms = ms;
    L.ready = true;
  } catch (...) {
    // the locals are gone with their memory; a failed allocation leaves HIP's last-error word set,
    // which the next launch check of this call would otherwise take for its own
    (void)hipGetLastError();
    hip::block_cache_t::instance().trim();
    if (std::getenv("GRX_DEBUG"))
      std::fprintf(stderr, "[grx] sssp pull rows: not built (the build failed), this call pushes\n");
    return nullptr;
  }
  hip::block_cache_t::instance().trim();  // the sort's key buffers, see grx_graph_rmat
  if (std::getenv("GRX_DEBUG"))
    std::fprintf(stderr, "[grx] sssp pull rows: %lld records sorted in %.3f ms, %llu bytes\n", (long long)nnz,
                 (double)L.build_ms, (unsigned long long)(nnz * 8 + (std::size_t)g->n_rows * 4));
  return &L;
}

}  // namespace essentials_amd

extern "C" int grx_sssp(grx_context_t ctx, grx_graph_t g, int32_t source, float* d_distances,
                        int32_t* /*d_predecessors*/, const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g || !d_distances)
    return invalid("grx_sssp: NULL argument");
  if (source < 0 || source >= g->n_rows)
    return invalid("grx_sssp: source out of range");
  grx_options o = effective_options(opt);
  return guarded([&] {
    return with_load_balance(o.load_balance, [&](auto lb_tag) -> int {
      constexpr auto lb = decltype(lb_tag)::value;
      using problem_type = clients::sssp_problem_t<graph_type>;
      using enactor_type = clients::sssp_enactor_t<problem_type, lb>;
      scoped_options scope(ctx->single(), &o);
      // hot-first renumbered copy, distances delivered in the caller's numbering (see grx_bfs); the
      // reference's two-pass formulation and the every-edge form keep the caller's graph
      const run_graph_t run = run_graph(ctx, g, !o.sssp_two_pass && !o.call_every_edge && !o.holes_layout);
      graph_type G = run.on->view();
      problem_type problem(G, run.vertex(source), d_distances, ctx->mc);
      problem.scatter_to = run.scatter_to;
      problem.gather_from = run.gather_from;
      // one 64-bit label per vertex (one RMW per improvement) while 8 bytes per vertex stay
      // cache-sized; beyond that the doubled label footprint costs more lookups that miss than the
      // saved RMWs are worth.  Measured crossover on R-MAT (tools/sssp_packed_vs_words.py, mean
      // enact of 3 sources, packed / two words): scale 20 1.25 / 1.42 ms, 22 2.92 / 3.11, 23 5.56 /
      // 5.46, 24 12.8 / 11.0, 26 58.2 / 53.5.  GRX_SSSP_PACKED=0/1 overrides; the reference's
      // two-pass formulation keeps its two arrays.
      const bool packed = env_flag("GRX_SSSP_PACKED", g->n_rows <= essentials_amd::packed_sssp_max_vertices());
      problem.packed_labels = packed && o.sssp_two_pass == 0;
      // the unpacking pass at the end of a packed run also counts what the run reached
      problem.collect_reach = stats != nullptr && problem.packed_labels;
      // wide pending sets are expanded nearest half first (clients.hxx, select_near): where the label
      // scan exists and the run ends by itself on one GPU; GRX_SSSP_NEAR=0 switches it off
      problem.near_far = env_flag("GRX_SSSP_NEAR", true) && problem.packed_labels &&
                         lb == operators::load_balance_t::block_mapped && !o.call_every_edge &&
                         !o.holes_layout && o.max_iterations == 0 && !ctx->mc->communicator().attached() &&
                         (unsigned long long)G.get_number_of_edges() < (1ull << 32);
      // ... and on a graph KNOWN to be its own transpose with equal weights the scanning wide rounds
      // of such a run pull over its weight-sorted rows (clients.hxx, pull_round), built here on first
      // use, outside enact(); GRX_SSSP_PULL=0 switches it off.  No check is run for this.
      // Not for a graph no round of which can ever follow a selection: a selection needs pending work
      // of both thresholds, and no pending set holds more edges than the graph.
      const auto& ctx_options = ctx->single().options();
      const unsigned long long selects_from = std::max(ctx_options.sssp_near_min_work, ctx_options.label_scan_min_work);
      const bool may_pull = problem.near_far && env_flag("GRX_SSSP_PULL", true) &&
                            ctx_options.sssp_near_min_work != 0 && ctx_options.label_scan_min_work != 0 &&
                            (unsigned long long)G.get_number_of_edges() >= selects_from;
      if (may_pull)
        if (const auto* rows = light_rows(ctx, run.on)) {
          problem.light_rows.records = rows->records.data();
          problem.light_rows.lightest = rows->lightest.data();
        }
      problem.init();
      problem.reset();
      enactor_properties_t props;
      if (o.frontier_sizing_factor > 0)
        props.frontier_sizing_factor = o.frontier_sizing_factor;
      enactor_type enactor(&problem, ctx->mc, props);
      enactor.max_iterations = o.max_iterations;
      enactor.two_pass = o.sssp_two_pass != 0;
      enactor.bound_filter = env_flag("GRX_SSSP_BOUND_FILTER", o.call_every_edge == 0);
      enactor.early_live = env_flag("GRX_SSSP_EARLY_LIVE", enactor.early_live);
      enactor.bound_from = (int)env_or("GRX_SSSP_BOUND_FROM", enactor.bound_from, INT_MIN, INT_MAX);
      if (const char* e = std::getenv("GRX_SSSP_NEAR_FRAC"))  // for the sweep behind the default
        enactor.near_frac = std::min(1.0, std::max(1.0 / 64, std::atof(e)));
      if (const char* e = std::getenv("GRX_SSSP_PULL_ALPHA"))  // 0: every eligible round pulls
        enactor.pull_alpha = std::max(0.0, std::atof(e));
      const float ms = enactor.enact();
      if (stats) {
        run_stats(stats, ms, enactor.iteration, ctx->single());
        level_stats(stats, problem.log);
        stats->pull_iterations = enactor.pull_iterations;
        // the first frontier ({source}) carries no work hint: add the source's own degree
        const unsigned long long* facts = ctx->single().workspace().run_facts();
        if (problem.collect_reach && facts[3] == 1ull) {  // left in pinned memory by unpack()
          stats->vertices_reached = (int64_t)facts[1];
          stats->edges_traversed = (int64_t)facts[2];
          stats->edges_expanded = problem.log.edges_expanded + (long long)facts[0];
        } else {
          stats->edges_expanded =
              problem.log.edges_expanded + reach_stats(g, d_distances, FLT_MAX, source, ctx->single(), stats);
        }
      }
      return (int)GRX_OK;
    });
  });
}

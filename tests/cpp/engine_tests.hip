// engine_tests.hip -- C++-level checks of the header surface that the C ABI does not reach:
// frontier_t methods, parallel_for, enactor-overload operators (swap rules), explicit-frontier
// advance (the form reference algorithms/bc.hxx:140-181 uses), batch, multi-context rejection,
// and (when built with -DGRX_ADVANCE_LB_OVERRIDE=...) the schedule override.
// Self-checking: expected values are computed by plain host loops below.  Exit code 0 = pass.
// With `--dump FILE` the inputs and the DEVICE results of the operator sections (parallel_for,
// explicit-frontier advance per schedule, filters, uniquify) are also written as JSON, and
// tests/test_gpu_cpp_surface.py compares them with oracle/ -- the binary is not its own only judge.
#include <gunrock/algorithms/algorithms.hxx>
#include <gunrock/graph/reorder.hxx>
#include <gunrock/hip/algorithms.hxx>
#include <gunrock/hip/kernels/generation_queue.hxx>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <set>
#include <string>
#include <vector>

using namespace gunrock;
using vertex_t = int;
using edge_t = int;
using weight_t = float;

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);         \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

struct host_graph {
  int n;
  std::vector<int> ap, aj;
  std::vector<float> ax;
};

// deterministic pseudo-random multigraph with a hub (vertex 0) and isolated vertices
static host_graph make_graph(int n, int avg) {
  host_graph g;
  g.n = n;
  g.ap.assign(n + 1, 0);
  unsigned s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  std::vector<std::vector<int>> adj(n);
  for (int v = 0; v < n; ++v) {
    int d = (v == 0) ? std::min(n - 1, 5000) : (v % 7 == 3 ? 0 : (int)(rnd() % (2 * avg)));
    for (int k = 0; k < d; ++k)
      adj[v].push_back((int)(rnd() % n));
  }
  for (int v = 0; v < n; ++v) {
    g.ap[v + 1] = g.ap[v] + (int)adj[v].size();
    for (int c : adj[v]) { g.aj.push_back(c); g.ax.push_back(1.0f + (float)(c % 5)); }
  }
  return g;
}

template <typename T>
static hip::device_array_t<T> upload(const std::vector<T>& h) {
  hip::device_array_t<T> d;
  d.assign(h.data(), h.size());
  return d;
}

// a minimal problem/enactor pair so that the enactor overloads can be exercised
template <typename graph_t>
struct toy_problem_t : gunrock::problem_t<graph_t> {
  using gunrock::problem_t<graph_t>::problem_t;
  void init() override {}
  void reset() override {}
};
template <typename problem_type>
struct toy_enactor_t : gunrock::enactor_t<problem_type> {
  using gunrock::enactor_t<problem_type>::enactor_t;
  void loop(gcuda::multi_context_t&) override {}
};

// one small kernel per workgroup helper of hip/primitives.hxx, hip/kernels/row_walk.hxx and
// hip/kernels/generation_queue.hxx
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) block_sum_probe(const unsigned long long* in, unsigned long long* out) {
  __shared__ unsigned long long s_wave[BLOCK / hip::wave_size];
  const unsigned long long total = hip::block_sum<BLOCK>(in[threadIdx.x], s_wave);
  if (threadIdx.x == 0)
    *out = total;
}
__global__ void __launch_bounds__(64) wave_min_probe(const unsigned* in, unsigned* out) {
  out[threadIdx.x] = hip::wave_min(in[threadIdx.x]);
}
__global__ void __launch_bounds__(64) prefix_owner_probe(const int* pre, int cnt, int n_t, int* out) {
  if ((int)threadIdx.x < n_t)
    out[threadIdx.x] = hip::prefix_owner(pre, cnt, (int)threadIdx.x);
}
__global__ void __launch_bounds__(64) push_big_probe(int* big_n, int2* big, int v, int d) {
  if (threadIdx.x == 0)
    hip::kernels::push_big_segments<4096>(big_n, big, v, d);
}

// two wavefronts; thread t appends vertex t when ready[t]
template <bool NARROW>
__global__ void __launch_bounds__(128) queue_append_probe(const int* ready, const int* ap, int* queue, int n, int* tail,
                                                          unsigned long long* degsum) {
  const hip::kernels::queue_sink_t sink{queue, n, tail, degsum};
  unsigned long long dsum = 0;
  hip::kernels::queue_append<NARROW>(ready[threadIdx.x] != 0, (int)threadIdx.x, ap, sink, dsum);
  hip::kernels::queue_flush(dsum, degsum);
}
// queue[0, cnt) as one chunk: visits[e] counts the live calls at position e, owners[e] keeps their owner
__global__ void __launch_bounds__(256) queue_walk_probe(const int* ap, const int* queue, int cnt, int big_row, int* big,
                                                        int* big_n, int* visits, int* owners, int* dead, int* entries) {
  __shared__ int s_pre[256], s_base[256], s_wave[256 / hip::wave_size + 1];
  const int P = hip::kernels::queue_walk<256, false>(
      ap, queue, 0, cnt, s_pre, s_base, s_wave,
      [&](int v, int, int& d) { hip::kernels::queue_divert_big(v, d, big_row, big, big_n); },
      [&](bool live, int o, int e) {
        if (live) {
          atomicAdd(&visits[e], 1);
          owners[e] = o;
        } else {
          atomicAdd(dead, 1);
        }
      });
  if (threadIdx.x == 0)
    *entries = P;
}
// a chain: the generation {v} walks row v and appends v + 1 while there is one
__global__ void __launch_bounds__(1024) narrow_generations_probe(const hip::kernels::queue_counters_t* ctr, const int* ap,
                                                                 int* queue, int n, unsigned long long max_edges,
                                                                 hip::kernels::narrow_result_t* out) {
  __shared__ int s_tail;
  __shared__ unsigned long long s_dsum;
  const auto r = hip::kernels::narrow_generations(
      ctr, queue, n, 1024, max_edges, &s_tail, &s_dsum,
      [&](int head, int, const hip::kernels::queue_sink_t& sink, unsigned long long& dsum) {
        const int v = hip::load_relaxed(sink.queue + head);
        __syncthreads();  // as behind a walk's prefix sum: the loop's reset of the degree sum is over
        hip::kernels::queue_append<true>(threadIdx.x == 0 && v + 1 < n, v + 1, ap, sink, dsum);
        __syncthreads();
        return ap[v + 1] - ap[v];
      });
  if (threadIdx.x == 0)
    *out = r;
}

static FILE* dump = nullptr;
template <typename T>
static void dump_array(const char* key, const std::vector<T>& v, bool last = false) {
  if (!dump)
    return;
  std::fprintf(dump, "\"%s\": [", key);
  for (std::size_t i = 0; i < v.size(); ++i)
    std::fprintf(dump, i ? ",%lld" : "%lld", (long long)v[i]);
  std::fprintf(dump, last ? "]\n" : "],\n");
}

int main(int argc, char** argv) {
  if (argc == 3 && std::strcmp(argv[1], "--dump") == 0) {
    dump = std::fopen(argv[2], "w");
    if (dump)
      std::fprintf(dump, "{\n");
  }
  auto mc = std::make_shared<gcuda::multi_context_t>(0);
  auto& ctx = *mc->get_context(0);
  using frontier_t = frontier::frontier_t<vertex_t, edge_t>;

  // ---- frontier_t -----------------------------------------------------------------------
  {
    frontier_t f;
    CHECK(f.is_empty() && f.get_number_of_elements() == 0);
    for (int i = 0; i < 200; ++i) f.push_back(i * 3);   // grows past its first allocation
    auto h = f.to_host();
    CHECK(h.size() == 200 && h[0] == 0 && h[199] == 597);
    f.reserve(100000);                                  // contents survive a reserve
    CHECK(f.get_capacity() >= 100000 && f.to_host() == h);
    f.resize(210);                                      // new slots are invalid
    h = f.to_host();
    CHECK(h.size() == 210 && h[205] == -1 && h[199] == 597);
    f.sequence(7, 1000, ctx.stream());
    ctx.synchronize();
    h = f.to_host();
    CHECK(h.size() == 1000 && h[0] == 7 && h[999] == 1006);
    f.fill(42, ctx.stream());
    ctx.synchronize();
    h = f.to_host();
    CHECK(std::all_of(h.begin(), h.end(), [](int x) { return x == 42; }));
    std::vector<int> mixed = {5, -1, 3, 9, 3, 0, 7};
    frontier_t m;
    for (int x : mixed) m.push_back(x);
    m.sort(sort::order_t::ascending, ctx.stream());
    std::sort(mixed.begin(), mixed.end());
    CHECK(m.to_host() == mixed);
    m.sort(sort::order_t::descending, ctx.stream());
    std::reverse(mixed.begin(), mixed.end());
    CHECK(m.to_host() == mixed);
    CHECK(m.work_hint() == frontier_t::unknown_work);
  }

  host_graph hg = make_graph(20000, 12);
  auto d_ap = upload(hg.ap);
  auto d_aj = upload(hg.aj);
  auto d_ax = upload(hg.ax);
  auto G = graph::build::from_csr<memory_space_t::device, graph::view_t::csr>(
      hg.n, hg.n, (int)hg.aj.size(), d_ap.data(), d_aj.data(), d_ax.data());
  using graph_t = decltype(G);
  CHECK(G.get_number_of_vertices() == hg.n && G.get_number_of_edges() == (int)hg.aj.size());
  dump_array("row_offsets", hg.ap);
  dump_array("column_indices", hg.aj);
  {
    std::vector<int> w(hg.ax.begin(), hg.ax.end());  // small integers
    dump_array("values", w);
  }

  // ---- parallel_for -----------------------------------------------------------------------
  {
    hip::device_array_t<int> deg(hg.n);
    int* pdeg = deg.data();
    auto per_vertex = [G, pdeg] __device__(vertex_t const& v) { pdeg[v] = G.get_number_of_neighbors(v); };
    operators::parallel_for::execute<operators::parallel_for_each_t::vertex>(G, per_vertex, *mc);
    auto h = deg.to_host();
    dump_array("parallel_for_vertex_degrees", h);
    bool ok = true;
    for (int v = 0; v < hg.n; ++v) ok &= h[v] == hg.ap[v + 1] - hg.ap[v];
    CHECK(ok);
    hip::device_array_t<int> src(hg.aj.size());
    int* psrc = src.data();
    auto per_edge = [G, psrc] __device__(edge_t const& e) { psrc[e] = G.get_source_vertex(e); };
    operators::parallel_for::execute<operators::parallel_for_each_t::edge>(G, per_edge, *mc);
    auto hs = src.to_host();
    dump_array("parallel_for_edge_sources", hs);
    ok = true;
    for (int v = 0; v < hg.n; ++v)
      for (int e = hg.ap[v]; e < hg.ap[v + 1]; ++e) ok &= hs[e] == v;
    CHECK(ok);
    hip::device_array_t<float> acc(1);
    acc.zero();
    float* pacc = acc.data();
    auto per_weight = [pacc] __device__(weight_t const& w) { math::atomic::add(pacc, w); };
    operators::parallel_for::execute<operators::parallel_for_each_t::weight>(G, per_weight, *mc);
    CHECK(acc.to_host()[0] == std::accumulate(hg.ax.begin(), hg.ax.end(), 0.0f));  // small ints: exact
    frontier_t f;
    for (int x : {4, -1, 9, 4}) f.push_back(x);
    hip::device_array_t<int> hits(hg.n);
    hits.zero();
    int* phits = hits.data();
    auto per_elem = [phits] __device__(vertex_t const& v) { math::atomic::add(&phits[v], 1); };
    operators::parallel_for::execute<operators::parallel_for_each_t::element>(f, per_elem, *mc);
    auto hh = hits.to_host();
    CHECK(hh[4] == 2 && hh[9] == 1 && std::accumulate(hh.begin(), hh.end(), 0) == 3);
  }

  // ---- explicit-frontier advance, every schedule, vertices->vertices and vertices->none --------
  std::vector<int> fin_h;
  for (int v = 0; v < hg.n; v += 3) fin_h.push_back(v);
  fin_h.push_back(-1);
  fin_h.push_back(0);  // the hub twice
  dump_array("advance_frontier", fin_h);
  std::vector<long long> want_hits(hg.n, 0);
  std::multiset<int> want_out;
  for (int v : fin_h) {
    if (v < 0) continue;
    for (int e = hg.ap[v]; e < hg.ap[v + 1]; ++e) {
      want_hits[hg.aj[e]] += 1;
      if ((v + hg.aj[e]) % 2 == 0) want_out.insert(hg.aj[e]);
    }
  }
  auto run_schedule = [&](auto lb_tag, const char* name) {
    constexpr operators::load_balance_t lb = decltype(lb_tag)::value;
    frontier_t fin, fout;
    for (int v : fin_h) fin.push_back(v);
    hip::device_array_t<int> hits(hg.n);
    hits.zero();
    int* ph = hits.data();
    hip::device_array_t<edge_t> segments;
    auto op = [ph] __host__ __device__(vertex_t const& s, vertex_t const& d, edge_t const& e,
                                       weight_t const& w) -> bool {
      math::atomic::add(&ph[d], 1);
      return (s + d) % 2 == 0;
    };
    operators::advance::execute<lb, operators::advance_direction_t::forward,
                                operators::advance_io_type_t::vertices,
                                operators::advance_io_type_t::vertices>(G, op, &fin, &fout, segments, *mc);
    auto out = fout.to_host();
    std::multiset<int> got(out.begin(), out.end());
    got.erase(-1);
    auto hh = hits.to_host();
    {
      std::vector<int> sorted_out(got.begin(), got.end());
      dump_array((std::string("advance_output_") + name).c_str(), sorted_out);
      dump_array((std::string("advance_calls_per_destination_") + name).c_str(), hh);
    }
    bool ok = true;
    for (int v = 0; v < hg.n; ++v) ok &= hh[v] == want_hits[v];
    if (!(ok && got == want_out)) { std::printf("FAIL schedule %s (vertices->vertices)\n", name); ++failures; }
    CHECK(fout.work_hint() != frontier_t::unknown_work);
    hits.zero();
    operators::advance::execute<lb, operators::advance_direction_t::forward,
                                operators::advance_io_type_t::vertices,
                                operators::advance_io_type_t::none>(G, op, &fin, &fout, segments, *mc);
    hh = hits.to_host();
    ok = true;
    for (int v = 0; v < hg.n; ++v) ok &= hh[v] == want_hits[v];
    if (!ok) { std::printf("FAIL schedule %s (vertices->none)\n", name); ++failures; }
  };
  using lbt = operators::load_balance_t;
  run_schedule(std::integral_constant<lbt, lbt::merge_path>(), "merge_path");
  run_schedule(std::integral_constant<lbt, lbt::merge_path_v2>(), "merge_path_v2");
  run_schedule(std::integral_constant<lbt, lbt::block_mapped>(), "block_mapped");
  run_schedule(std::integral_constant<lbt, lbt::thread_mapped>(), "thread_mapped");
  run_schedule(std::integral_constant<lbt, lbt::warp_mapped>(), "warp_mapped");
  run_schedule(std::integral_constant<lbt, lbt::bucketing>(), "bucketing");
  run_schedule(std::integral_constant<lbt, lbt::work_stealing>(), "work_stealing");

  // ---- settled destinations (operators/settled.hxx): bitmap + pure predicate in front of the functor
  {
    auto* ctx0 = mc->get_context(0);
    const auto saved = ctx0->options();
    ctx0->options().settled_min_work = 1;  // take the wide-level form for this small frontier too
    frontier_t fin, fout;
    for (int v : fin_h) fin.push_back(v);
    unsigned long long work = 0;  // the form is chosen by the frontier's known work
    for (int v : fin_h)
      if (v >= 0) work += (unsigned long long)(hg.ap[v + 1] - hg.ap[v]);
    fin.set_work_hint(work);
    hip::device_array_t<int> hits(hg.n);
    hits.zero();
    int* ph = hits.data();
    hip::device_array_t<edge_t> segments;
    auto op = [ph] __host__ __device__(vertex_t const& s, vertex_t const& d, edge_t const& e,
                                       weight_t const& w) -> bool {
      math::atomic::add(&ph[d], 1);
      return (s + d) % 2 == 0;
    };
    // the client names d % 3 == 0 through the bitmap and d % 5 == 0 through the predicate
    operators::advance::settled_filter_t<vertex_t> named;
    named.rebuild((std::size_t)hg.n, [] __device__(vertex_t v) { return v % 3 == 0; }, *ctx0);
    auto by_rule = [] __host__ __device__(vertex_t const& v) -> bool { return v % 5 == 0; };
    auto hinted = operators::advance::with_settled(op, named.view(), by_rule);
#ifdef GRX_ADVANCE_LB_OVERRIDE  // another schedule runs: it has no LDS filter and must ignore the hint
    auto is_named = [](int) { return false; };
#else
    auto is_named = [](int d) { return d % 3 == 0 || d % 5 == 0; };
#endif
    constexpr auto lb = operators::load_balance_t::block_mapped;
    operators::advance::execute<lb, operators::advance_direction_t::forward,
                                operators::advance_io_type_t::vertices,
                                operators::advance_io_type_t::vertices>(G, hinted, &fin, &fout, segments, *mc);
    auto out = fout.to_host();
    std::multiset<int> got(out.begin(), out.end()), want;
    got.erase(-1);
    for (int d : want_out)
      if (!is_named(d)) want.insert(d);
    auto hh = hits.to_host();
    bool ok = true;
    // contract: exactly once per edge into a destination that was not named, at most once per edge
    // otherwise; THIS kernel skips every named destination, which also proves it ran
    for (int v = 0; v < hg.n; ++v) ok &= is_named(v) ? hh[v] == 0 : hh[v] == want_hits[v];
    if (!(ok && got == want)) { std::printf("FAIL settled hint (vertices->vertices)\n"); ++failures; }
    {
      std::vector<int> sorted_out(got.begin(), got.end());
      dump_array("advance_settled_output", sorted_out);
      dump_array("advance_settled_calls_per_destination", hh);
    }
    hits.zero();
    operators::advance::execute<lb, operators::advance_direction_t::forward,
                                operators::advance_io_type_t::vertices,
                                operators::advance_io_type_t::none>(G, hinted, &fin, &fout, segments, *mc);
    hh = hits.to_host();
    ok = true;
    for (int v = 0; v < hg.n; ++v) ok &= is_named(v) ? hh[v] == 0 : hh[v] == want_hits[v];
    if (!ok) { std::printf("FAIL settled hint (vertices->none)\n"); ++failures; }
    // the per-edge form: a pure predicate of (src, dst, edge, weight), no bitmap
    {
      auto by_edge = [] __host__ __device__(vertex_t const& s, vertex_t const& d, edge_t const& e,
                                            weight_t const& w) -> bool { return (s + 2 * d + e) % 3 == 0; };
      auto edge_hinted = operators::advance::with_rejects<vertex_t>(op, by_edge);
      std::vector<long long> want_calls(hg.n, 0);
      std::multiset<int> want_kept;
      for (int v : fin_h) {
        if (v < 0) continue;
        for (int e = hg.ap[v]; e < hg.ap[v + 1]; ++e) {
#ifndef GRX_ADVANCE_LB_OVERRIDE
          if ((v + 2 * hg.aj[e] + e) % 3 == 0) continue;
#endif
          want_calls[hg.aj[e]] += 1;
          if ((v + hg.aj[e]) % 2 == 0) want_kept.insert(hg.aj[e]);
        }
      }
      hits.zero();
      operators::advance::execute<lb, operators::advance_direction_t::forward,
                                  operators::advance_io_type_t::vertices,
                                  operators::advance_io_type_t::vertices>(G, edge_hinted, &fin, &fout, segments, *mc);
      auto o2 = fout.to_host();
      std::multiset<int> got2(o2.begin(), o2.end());
      got2.erase(-1);
      hh = hits.to_host();
      ok = true;
      for (int v = 0; v < hg.n; ++v) ok &= hh[v] == want_calls[v];
      if (!(ok && got2 == want_kept)) { std::printf("FAIL rejected-edge hint (vertices->vertices)\n"); ++failures; }
    }
    // switched off, or on a schedule without the LDS filter, the functor sees every edge
    ctx0->options().settled_filter = false;
    hits.zero();
    operators::advance::execute<lb, operators::advance_direction_t::forward,
                                operators::advance_io_type_t::vertices,
                                operators::advance_io_type_t::none>(G, hinted, &fin, &fout, segments, *mc);
    hh = hits.to_host();
    ok = true;
    for (int v = 0; v < hg.n; ++v) ok &= hh[v] == want_hits[v];
    ctx0->options().settled_filter = true;
    hits.zero();
    operators::advance::execute<operators::load_balance_t::merge_path, operators::advance_direction_t::forward,
                                operators::advance_io_type_t::vertices,
                                operators::advance_io_type_t::none>(G, hinted, &fin, &fout, segments, *mc);
    hh = hits.to_host();
    for (int v = 0; v < hg.n; ++v) ok &= hh[v] == want_hits[v];
    if (!ok) { std::printf("FAIL settled hint ignored where it must be\n"); ++failures; }
    ctx0->options() = saved;
  }

  // ---- round-3 engine extensions: select_range, with_bounds, hot_first -----------------------------
  {
    auto* ctx0 = mc->get_context(0);
    const auto saved = ctx0->options();
    // (1) operators::filter::select_range == sequence(0, n) + filter::predicated as a SET, with the
    //     selection's degree sum as work hint, ascending runs, and the two side products
    frontier_t picked;
    hip::device_array_t<int> touched(hg.n);
    touched.zero();
    int* pt = touched.data();
    const std::size_t bit_limit = ((std::size_t)hg.n / 64) * 64;
    hip::device_array_t<unsigned long long> words(bit_limit / 64);
    auto want_v = [] __host__ __device__(vertex_t const& v) -> bool { return v % 3 == 1; };
    auto each = [pt] __device__(vertex_t const& v) { pt[v] += 1; };
    auto bit = [] __device__(vertex_t const& v) -> bool { return v % 7 == 0; };
    operators::filter::select_range(G, (std::size_t)hg.n, want_v, picked, *ctx0, each, bit, words.data(), bit_limit);
    auto got = picked.to_host();
    std::vector<int> expect;
    unsigned long long expect_work = 0;
    for (int v = 0; v < hg.n; ++v)
      if (v % 3 == 1) { expect.push_back(v); expect_work += (unsigned long long)(hg.ap[v + 1] - hg.ap[v]); }
    bool runs_ascend = true;  // inside every run of one 8192-id chunk
    for (std::size_t i = 1; i < got.size(); ++i)
      if (got[i] < got[i - 1] && got[i] / 8192 == got[i - 1] / 8192) runs_ascend = false;
    auto sorted_got = got;
    std::sort(sorted_got.begin(), sorted_got.end());
    CHECK(sorted_got == expect && runs_ascend);
    CHECK(picked.work_hint() == expect_work && picked.ascending());
    auto th = touched.to_host();
    CHECK(std::all_of(th.begin(), th.end(), [](int x) { return x == 1; }));  // `each`: once per id
    auto wh = words.to_host();
    bool bits_ok = true;
    for (std::size_t v = 0; v < bit_limit; ++v) bits_ok &= (((wh[v / 64] >> (v % 64)) & 1ull) != 0) == (v % 7 == 0);
    CHECK(bits_ok);
    dump_array("select_range_output", sorted_got);
    dump_array("select_range_work_hint", std::vector<long long>{(long long)picked.work_hint()});
    // an ascending frontier is dealt across the tiles of the wide-level kernel: same calls, same set
    {
      ctx0->options().settled_min_work = 1;
      hip::device_array_t<int> hits(hg.n);
      hits.zero();
      int* ph = hits.data();
      auto count = [ph] __host__ __device__(vertex_t const& s, vertex_t const& d, edge_t const& e,
                                            weight_t const& w) -> bool {
        math::atomic::add(&ph[d], 1);
        return (s + d) % 2 == 0;
      };
      operators::advance::settled_filter_t<vertex_t> none_named;
      none_named.rebuild((std::size_t)hg.n, [] __device__(vertex_t) { return false; }, *ctx0);
      frontier_t out_f;
      hip::device_array_t<edge_t> seg;
      CHECK(picked.ascending());
      operators::advance::execute<operators::load_balance_t::block_mapped, operators::advance_direction_t::forward,
                                  operators::advance_io_type_t::vertices,
                                  operators::advance_io_type_t::vertices>(
          G, operators::advance::with_settled(count, none_named.view()), &picked, &out_f, seg, *mc);
      std::vector<long long> want_calls(hg.n, 0);
      std::multiset<int> want_kept;
      for (int v : expect)
        for (int e = hg.ap[v]; e < hg.ap[v + 1]; ++e) {
          want_calls[hg.aj[e]] += 1;
          if ((v + hg.aj[e]) % 2 == 0) want_kept.insert(hg.aj[e]);
        }
      auto hh = hits.to_host();
      auto oo = out_f.to_host();
      std::multiset<int> got_kept(oo.begin(), oo.end());
      bool ok = got_kept == want_kept;
      for (int v = 0; v < hg.n; ++v) ok &= hh[v] == want_calls[v];
#ifndef GRX_ADVANCE_LB_OVERRIDE
      if (!ok) { std::printf("FAIL ascending frontier dealt across tiles\n"); ++failures; }
#else
      CHECK(ok);
#endif
    }
    // (2) operators::advance::with_bounds: a min-relaxation with a 2-byte bound image gives the labels and
    //     the improved set of the plain functor
    {
      ctx0->options().settled_min_work = 1;
      const unsigned far = 1u << 30;
      std::vector<unsigned> init(hg.n, far);
      for (int v : fin_h) if (v >= 0) init[v] = (unsigned)(v % 50);
      auto run = [&](bool bounded, std::vector<unsigned>& labels_out, std::multiset<int>& improved) {
        auto d_label = upload(init);
        auto d_source = upload(init);  // what a source hands on is read from a copy: one Jacobi round, the
        unsigned* lab = d_label.data();  // same labels whatever order the engine relaxes in
        const unsigned* from = d_source.data();
        hip::device_array_t<unsigned short> bound16(hg.n);
        unsigned short* b16 = bound16.data();
        hip::for_each_index((std::size_t)hg.n, [lab, b16] __device__(std::size_t i) {
          b16[i] = lab[i] >= 0xffffu ? (unsigned short)0xffffu : (unsigned short)lab[i];  // exact for small labels
        }, ctx.stream());
        auto relax = [lab, from] __host__ __device__(vertex_t const& s, vertex_t const& d, edge_t const& e,
                                                     weight_t const& w) -> bool {
          const unsigned through = from[s] + (unsigned)w;
          return through < math::atomic::min(&lab[d], through);
        };
        auto cached = [from] __device__(vertex_t const& s, vertex_t const& d, edge_t const& e, weight_t const& w,
                                        unsigned short const& b) -> bool {
          return b != 0xffffu && from[s] + (unsigned)w >= (unsigned)b;
        };
        auto pred = [cached, b16] __device__(vertex_t const& s, vertex_t const& d, edge_t const& e,
                                             weight_t const& w) -> bool { return cached(s, d, e, w, b16[d]); };
        frontier_t fin2, fout2;
        for (int v : fin_h) fin2.push_back(v);
        unsigned long long work = 0;
        for (int v : fin_h) if (v >= 0) work += (unsigned long long)(hg.ap[v + 1] - hg.ap[v]);
        fin2.set_work_hint(work);
        hip::device_array_t<edge_t> seg;
        constexpr auto lb = operators::load_balance_t::block_mapped;
        if (bounded)
          operators::advance::execute<lb, operators::advance_direction_t::forward,
                                      operators::advance_io_type_t::vertices,
                                      operators::advance_io_type_t::vertices>(
              G, operators::advance::with_bounds<vertex_t>(relax, pred, cached, b16, (std::size_t)hg.n), &fin2,
              &fout2, seg, *mc);
        else
          operators::advance::execute<lb, operators::advance_direction_t::forward,
                                      operators::advance_io_type_t::vertices,
                                      operators::advance_io_type_t::vertices>(G, relax, &fin2, &fout2, seg, *mc);
        labels_out = d_label.to_host();
        auto o = fout2.to_host();
        improved = std::multiset<int>(o.begin(), o.end());
      };
      std::vector<unsigned> plain_labels, bounded_labels;
      std::multiset<int> plain_out, bounded_out;
      run(false, plain_labels, plain_out);
      run(true, bounded_labels, bounded_out);
      // the labels are a min over the same candidates whatever the order; the emitted multiset is not
      // (which of several improvers of a vertex "wins" more than once depends on timing): compare sets
      CHECK(plain_labels == bounded_labels);
      CHECK(std::set<int>(plain_out.begin(), plain_out.end()) == std::set<int>(bounded_out.begin(), bounded_out.end()));
      std::vector<long long> as_ll(bounded_labels.begin(), bounded_labels.end());
      dump_array("with_bounds_initial_labels", std::vector<long long>(init.begin(), init.end()));
      dump_array("with_bounds_labels", as_ll);
    }
    // (3) graph::build::hot_first: an isomorphic copy in descending degree order
    {
      unsigned long long max_deg = 0;
      for (int v = 0; v < hg.n; ++v) max_deg = std::max<unsigned long long>(max_deg, hg.ap[v + 1] - hg.ap[v]);
      auto R = graph::build::hot_first(G, *ctx0, max_deg);
      auto ro = R.offsets.to_host();
      auto rj = R.indices.to_host();
      auto rx = R.values.to_host();
      auto rank_of = R.rank_of.to_host();
      auto vertex_of = R.vertex_of.to_host();
      bool ok = ro[0] == 0 && ro[hg.n] == (int)hg.aj.size();
      for (int r = 0; r < hg.n && ok; ++r) {
        const int v = vertex_of[r];
        ok &= rank_of[v] == r;
        const int deg = ro[r + 1] - ro[r];
        ok &= deg == hg.ap[v + 1] - hg.ap[v];
        if (r) ok &= deg <= ro[r] - ro[r - 1];                                  // falling degrees
        if (r && deg == ro[r] - ro[r - 1]) ok &= vertex_of[r - 1] < v;          // ties keep the input order
        for (int k = 0; k < deg && ok; ++k)                                     // rows keep their edge order
          ok &= rj[ro[r] + k] == rank_of[hg.aj[hg.ap[v] + k]] && rx[ro[r] + k] == hg.ax[hg.ap[v] + k];
      }
      CHECK(ok);
      dump_array("hot_first_vertex_of", vertex_of);
      dump_array("hot_first_offsets", ro);
      dump_array("hot_first_indices", rj);
    }
    ctx0->options() = saved;
  }

  // ---- neighborreduce: per-vertex reduction over out-edges (reference neighborreduce.hxx:55-101) ---
  {
    using problem_type = toy_problem_t<graph_t>;
    problem_type P(G, mc);
    toy_enactor_t<problem_type> E(&P, mc);
    hip::device_array_t<float> y(hg.n);
    float* py = y.data();
    std::vector<float> xs(hg.n);
    for (int v = 0; v < hg.n; ++v) xs[v] = (float)(v % 7);     // small integers: float sums are exact
    auto d_x = upload(xs);
    const float* px = d_x.data();
    auto term = [G, px] __host__ __device__(edge_t e) -> float {
      return G.get_edge_weight(e) * px[G.get_destination_vertex(e)];
    };
    auto plus = [] __host__ __device__(float a, float b) -> float { return a + b; };
    operators::neighborreduce::execute(G, &E, py, term, plus, 0.0f, *mc);
    auto hy = y.to_host();
    bool ok = true;
    for (int v = 0; v < hg.n; ++v) {
      float want = 0;
      for (int e = hg.ap[v]; e < hg.ap[v + 1]; ++e) want += hg.ax[e] * xs[hg.aj[e]];
      ok &= hy[v] == want;
    }
    CHECK(ok);  // includes the hub row (5000 edges) and the edgeless rows (0)
    {
      std::vector<long long> as_int(hy.begin(), hy.end());
      dump_array("neighborreduce_sum_w_times_x", as_int);
    }
    // another monoid: maximum column id per row (-1 for an edgeless row)
    hip::device_array_t<int> mx(hg.n);
    auto col = [G] __host__ __device__(edge_t e) -> int { return G.get_destination_vertex(e); };
    auto maxi = [] __host__ __device__(int a, int b) -> int { return a > b ? a : b; };
    operators::neighborreduce::execute(G, &E, mx.data(), col, maxi, -1, *mc);
    auto hm = mx.to_host();
    ok = true;
    for (int v = 0; v < hg.n; ++v) {
      int want = -1;
      for (int e = hg.ap[v]; e < hg.ap[v + 1]; ++e) want = std::max(want, hg.aj[e]);
      ok &= hm[v] == want;
    }
    CHECK(ok);
  }

  // ---- whole-graph advance without an output, walked by destination (operators/by_destination.hxx)
  {
    using problem_type = toy_problem_t<graph_t>;
    auto* ctx0 = mc->get_context(0);
    const auto saved = ctx0->options();
    ctx0->options().by_destination_min_edges = 1;  // this small graph too
    const std::size_t nnz = hg.aj.size();
    hip::device_array_t<float> sums(hg.n);
    hip::device_array_t<int> calls(nnz);
    hip::device_array_t<int> wrong(1);
    float* ps = sums.data();
    int* pc = calls.data();
    int* pw = wrong.data();
    // pr.hxx's shape: one float atomic add per edge into the destination's word; every call also
    // proves it carries ITS edge's source / destination / weight and counts itself
    auto spread = [G, ps, pc, pw] __host__ __device__(vertex_t const& s, vertex_t const& d, edge_t const& e,
                                                       weight_t const& w) -> bool {
      if (G.get_destination_vertex(e) != d || G.get_edge_weight(e) != w || e < G.get_starting_edge(s) ||
          e >= G.get_starting_edge(s) + G.get_number_of_neighbors(s))
        math::atomic::add(pw, 1);
      math::atomic::add(pc + e, 1);
      math::atomic::add(ps + d, w * (float)(1 + s % 3));   // small integers: float sums are exact
      return false;
    };
    std::vector<float> want(hg.n, 0.0f);
    for (int v = 0; v < hg.n; ++v)
      for (int e = hg.ap[v]; e < hg.ap[v + 1]; ++e) want[hg.aj[e]] += hg.ax[e] * (float)(1 + v % 3);
    auto& cache = ctx0->workspace().by_destination();
    for (int run = 0; run < 2; ++run) {        // two enactors: the second finds the list built
      problem_type P(G, mc);
      toy_enactor_t<problem_type> E(&P, mc);
      for (int call = 0; call < 3; ++call) {   // row by row, then sorted (built on the second call)
        sums.zero(); calls.zero(); wrong.zero();
        operators::advance::execute<lbt::block_mapped, operators::advance_direction_t::forward,
                                    operators::advance_io_type_t::graph,
                                    operators::advance_io_type_t::none>(G, &E, spread, *mc);
        CHECK(cache.built == (run > 0 || call > 0));
        CHECK(wrong.to_host()[0] == 0);
        auto hc = calls.to_host();
        CHECK(std::all_of(hc.begin(), hc.end(), [](int c) { return c == 1; }));  // once per edge
        CHECK(sums.to_host() == want);
      }
    }
    // the same addresses with other contents are another graph: the remembered list is dropped
    std::vector<float> ax2 = hg.ax;
    for (std::size_t e = 0; e < nnz; e += 3) ax2[e] += 1.0f;
    auto d_ax_saved = upload(hg.ax);
    GRX_HIP_CHECK(hipMemcpy((void*)G.get_nonzero_values(), ax2.data(), nnz * sizeof(float), hipMemcpyHostToDevice));
    for (int v = 0; v < hg.n; ++v) want[v] = 0.0f;
    for (int v = 0; v < hg.n; ++v)
      for (int e = hg.ap[v]; e < hg.ap[v + 1]; ++e) want[hg.aj[e]] += ax2[e] * (float)(1 + v % 3);
    {
      problem_type P(G, mc);
      toy_enactor_t<problem_type> E(&P, mc);
      for (int call = 0; call < 3; ++call) {
        sums.zero(); calls.zero(); wrong.zero();
        operators::advance::execute<lbt::block_mapped, operators::advance_direction_t::forward,
                                    operators::advance_io_type_t::graph,
                                    operators::advance_io_type_t::none>(G, &E, spread, *mc);
        CHECK(cache.built == (call > 0));
        CHECK(wrong.to_host()[0] == 0);
        CHECK(sums.to_host() == want);
      }
    }
    GRX_HIP_CHECK(hipMemcpy((void*)G.get_nonzero_values(), hg.ax.data(), nnz * sizeof(float), hipMemcpyHostToDevice));
    {
      std::vector<long long> as_int(want.begin(), want.end());
      dump_array("by_destination_sums_reweighted", as_int);
    }
    // one enactor advancing over two graphs in turn: right sums from either, and after three
    // switches the operator stops sorting (and fingerprinting) lists for that enactor
    {
      auto d_ax2 = upload(ax2);
      auto G2 = graph::build::from_csr<memory_space_t::device, graph::view_t::csr>(
          hg.n, hg.n, (int)hg.aj.size(), d_ap.data(), d_aj.data(), d_ax2.data());
      std::vector<float> want1(hg.n, 0.0f);
      for (int v = 0; v < hg.n; ++v)
        for (int e = hg.ap[v]; e < hg.ap[v + 1]; ++e) want1[hg.aj[e]] += hg.ax[e] * (float)(1 + v % 3);
      auto spread2 = [G2, ps, pc, pw] __host__ __device__(vertex_t const& s, vertex_t const& d, edge_t const& e,
                                                           weight_t const& w) -> bool {
        if (G2.get_destination_vertex(e) != d || G2.get_edge_weight(e) != w)
          math::atomic::add(pw, 1);
        math::atomic::add(pc + e, 1);
        math::atomic::add(ps + d, w * (float)(1 + s % 3));
        return false;
      };
      problem_type P(G, mc);
      toy_enactor_t<problem_type> E(&P, mc);
      for (int call = 0; call < 10; ++call) {
        sums.zero(); calls.zero(); wrong.zero();
        if (call % 2 == 0)
          operators::advance::execute<lbt::block_mapped, operators::advance_direction_t::forward,
                                      operators::advance_io_type_t::graph,
                                      operators::advance_io_type_t::none>(G, &E, spread, *mc);
        else
          operators::advance::execute<lbt::block_mapped, operators::advance_direction_t::forward,
                                      operators::advance_io_type_t::graph,
                                      operators::advance_io_type_t::none>(G2, &E, spread2, *mc);
        CHECK(wrong.to_host()[0] == 0);
        CHECK(sums.to_host() == (call % 2 == 0 ? want1 : want));
        CHECK(!cache.built);  // never two calls in a row on one graph
      }
      CHECK(cache.switches >= 3 && cache.alternating_in == E.unique_id);
    }
    // math::atomic::add on floats combines runs of neighbouring lanes with the same address: the
    // totals are those of one add per lane, and the values returned for one word are the word's
    // values in ONE order of the adds (all ones added: 0, 1, 2, ... each exactly once)
    const int n_words = 97, n_lanes = 64 * 40;
    hip::device_array_t<float> words(n_words), olds(n_lanes);
    words.zero();
    float* pwords = words.data();
    float* polds = olds.data();
    auto pattern = [] __host__ __device__(int i) -> int {
      const int wave = i / 64, lane = i % 64;
      switch (wave % 5) {
        case 0: return 0;                       // the whole wave one word
        case 1: return lane / 7;                // runs of 7
        case 2: return lane;                    // no runs
        case 3: return (lane / 3) % 2;          // the same two words again and again, runs of 3
        default: return 50 + (lane * lane) / 97; // runs of falling length
      }
    };
    frontier_t lanes;
    lanes.sequence(0, (std::size_t)n_lanes, ctx.stream());
    operators::parallel_for::execute<operators::parallel_for_each_t::element>(
        lanes,
        [pwords, polds, pattern] __device__(vertex_t const& i) {
          if (i % 11 == 5) { polds[i] = -1.0f; return; }  // holes in the wave break runs
          polds[i] = math::atomic::add(pwords + pattern(i), 1.0f);
        },
        *mc);
    ctx.synchronize();
    auto hw = words.to_host();
    auto ho = olds.to_host();
    std::vector<std::vector<float>> seen(n_words);
    std::vector<float> count(n_words, 0.0f);
    for (int i = 0; i < n_lanes; ++i) {
      if (i % 11 == 5) continue;
      count[pattern(i)] += 1.0f;
      seen[pattern(i)].push_back(ho[i]);
    }
    bool ok = hw == count;
    for (int wd = 0; wd < n_words && ok; ++wd) {
      std::sort(seen[wd].begin(), seen[wd].end());
      for (std::size_t r = 0; r < seen[wd].size() && ok; ++r) ok &= seen[wd][r] == (float)r;
    }
    CHECK(ok);
    ctx0->options() = saved;
  }

  // ---- enactor overloads: which frontier is active afterwards ------------------------------
  {
    using problem_type = toy_problem_t<graph_t>;
    problem_type P(G, mc);
    toy_enactor_t<problem_type> E(&P, mc);
    auto* in0 = E.get_input_frontier();
    for (int x : {8, 2, 8, -1, 5, 2, 2}) in0->push_back(x);
    auto odd_or_8 = [] __host__ __device__(vertex_t const& v) -> bool { return v == 8 || (v & 1); };
    operators::filter::execute<operators::filter_algorithm_t::predicated>(G, &E, odd_or_8, *mc);
    CHECK(E.get_input_frontier() != in0);                        // swapped
    CHECK((E.get_input_frontier()->to_host() == std::vector<int>{8, 8, 5}));
    dump_array("filter_predicated_input", std::vector<int>{8, 2, 8, -1, 5, 2, 2});
    dump_array("filter_predicated_output", E.get_input_frontier()->to_host());
    operators::filter::execute<operators::filter_algorithm_t::bypass>(G, &E, odd_or_8, *mc, false);
    CHECK((E.get_output_frontier()->to_host() == std::vector<int>{8, 8, 5}));  // no swap asked
    auto* active = E.get_input_frontier();
    for (int x : {1, 5, 1}) active->push_back(x);                // 8 8 5 1 5 1
    operators::uniquify::execute<operators::uniquify_algorithm_t::unique>(&E, *mc);
    CHECK(E.get_input_frontier() == active);                     // in place: still the active one
    CHECK((active->to_host() == std::vector<int>{1, 5, 8}));
    dump_array("uniquify_input", std::vector<int>{8, 8, 5, 1, 5, 1});
    dump_array("uniquify_output", active->to_host());
    for (int x : {8, 8, 9}) active->push_back(x);                // 1 5 8 8 8 9
    operators::uniquify::execute<operators::uniquify_algorithm_t::unique_copy>(&E, *mc, true);
    CHECK(E.get_input_frontier() != active);                     // copy variant swaps
    CHECK((E.get_input_frontier()->to_host() == std::vector<int>{1, 5, 8, 9}));
    bool threw = false;
    try {
      operators::uniquify::execute<operators::uniquify_algorithm_t::unique>(&E, *mc, false, 150.0f);
    } catch (error::exception_t&) { threw = true; }
    CHECK(threw);
  }

  // ---- dense (bitmap) frontier view -----------------------------------------------------------
  {
    frontier::bitmap_frontier_t<vertex_t> bm(hg.n);
    frontier_t f;
    for (int x : {5, 64, -1, 5, 19999, 63, 128}) f.push_back(x);
    bm.assign(f, ctx);
    CHECK(bm.count(ctx) == 5);
    frontier_t back;
    bm.to_vector(back, ctx);
    CHECK((back.to_host() == std::vector<int>{5, 63, 64, 128, 19999}));
    bm.assign_if([] __device__(std::size_t v) { return v % 1000 == 7; }, ctx);
    CHECK(bm.count(ctx) == 20);
    bm.to_vector(back, ctx);
    auto hb = back.to_host();
    CHECK(hb.size() == 20 && hb[0] == 7 && hb[19] == 19007);
    hip::device_array_t<int> probe(3);
    int* pp = probe.data();
    auto view = bm.view();
    hip::for_each_index(3, [view, pp] __device__(std::size_t i) { pp[i] = view.test(i == 0 ? 7 : (i == 1 ? 8 : 19007)); }, ctx.stream());
    ctx.synchronize();
    CHECK((probe.to_host() == std::vector<int>{1, 0, 1}));
    bm.clear(ctx);
    CHECK(bm.count(ctx) == 0);
  }

  // ---- transpose (in-edge view) of a directed graph ------------------------------------------
  {
    auto T = graph::build::transpose(G, ctx);
    auto to = T.offsets.to_host();
    auto ti = T.indices.to_host();
    auto tv = T.values.to_host();
    auto te = T.edge_ids.to_host();
    std::vector<std::vector<std::pair<int, float>>> in(hg.n);
    for (int v = 0; v < hg.n; ++v)
      for (int e = hg.ap[v]; e < hg.ap[v + 1]; ++e) in[hg.aj[e]].push_back({v, hg.ax[e]});
    bool ok = to[0] == 0 && to[hg.n] == (int)hg.aj.size();
    for (int u = 0; u < hg.n && ok; ++u) {
      ok &= to[u + 1] - to[u] == (int)in[u].size();
      for (int k = 0; k < (int)in[u].size() && ok; ++k) {
        const int e = to[u] + k;                      // stable: ascending source order
        ok &= ti[e] == in[u][k].first && tv[e] == in[u][k].second && hg.aj[te[e]] == u;
      }
    }
    CHECK(ok);
    auto Gd = G;
    Gd.properties.directed = true;
    CHECK(!Gd.can_pull());
    T.attach_to(Gd);
    CHECK(Gd.can_pull() && Gd.has_in_edges());
  }

  // ---- the product's rocPRIM sort call sites at 4 K - 16 K elements ----------------------------
  // (frontier_t::sort, uniquify's sort, transpose's pair sort: the size range in which round 2's
  // removed experiment faulted; inputs and device results are dumped for the oracle comparison)
  {
    unsigned s = 2024u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    for (int n : {4096, 6000, 16384}) {
      std::vector<int> h(n);
      for (auto& x : h) x = (int)(rnd() % 3000u);
      frontier_t f;
      f.reserve(n);
      f.set_number_of_elements(n);
      GRX_HIP_CHECK(hipMemcpy(f.data(), h.data(), n * sizeof(int), hipMemcpyHostToDevice));
      f.sort(sort::order_t::ascending, ctx.stream());
      auto got = f.to_host();
      auto want = h;
      std::sort(want.begin(), want.end());
      CHECK(got == want);
      dump_array((std::string("sort_input_") + std::to_string(n)).c_str(), h);
      dump_array((std::string("sort_output_") + std::to_string(n)).c_str(), got);
      using problem_type = toy_problem_t<graph_t>;
      problem_type P(G, mc);
      toy_enactor_t<problem_type> E(&P, mc);
      auto* in0 = E.get_input_frontier();
      in0->reserve(n);
      in0->set_number_of_elements(n);
      GRX_HIP_CHECK(hipMemcpy(in0->data(), h.data(), n * sizeof(int), hipMemcpyHostToDevice));
      operators::uniquify::execute<operators::uniquify_algorithm_t::unique>(&E, *mc);
      auto uq = E.get_input_frontier()->to_host();
      std::set<int> distinct(h.begin(), h.end());
      CHECK(uq == std::vector<int>(distinct.begin(), distinct.end()));
      dump_array((std::string("uniquify_output_") + std::to_string(n)).c_str(), uq);
    }
    host_graph sg = make_graph(1500, 4);  // ~ 9 K edges
    auto s_ap = upload(sg.ap);
    auto s_aj = upload(sg.aj);
    auto s_ax = upload(sg.ax);
    auto SG = graph::build::from_csr<memory_space_t::device, graph::view_t::csr>(
        sg.n, sg.n, (int)sg.aj.size(), s_ap.data(), s_aj.data(), s_ax.data());
    auto T = graph::build::transpose(SG, ctx);
    CHECK(sg.aj.size() >= 4096 && sg.aj.size() <= 16384);
    dump_array("transpose_row_offsets", sg.ap);
    dump_array("transpose_column_indices", sg.aj);
    dump_array("transpose_result_offsets", T.offsets.to_host());
    dump_array("transpose_result_indices", T.indices.to_host());
    dump_array("transpose_result_edge_ids", T.edge_ids.to_host());
  }

  // ---- workgroup helpers shared by the cc / mst / kcore / tc kernels, each against a host loop -----
  {
    auto block_sum_of = [&](auto block_tag, const std::vector<unsigned long long>& in) {
      constexpr int BLOCK = decltype(block_tag)::value;
      auto d_in = upload(in);
      hip::device_array_t<unsigned long long> d_out(1);
      block_sum_probe<BLOCK><<<1, BLOCK, 0, ctx.stream()>>>(d_in.data(), d_out.data());
      ctx.synchronize();
      return d_out.to_host()[0];
    };
    auto check_block_sum = [&](auto block_tag) {
      constexpr int BLOCK = decltype(block_tag)::value;
      std::vector<unsigned long long> zeros(BLOCK, 0), last(BLOCK, 0), wide(BLOCK);
      last[BLOCK - 1] = 7;
      for (int i = 0; i < BLOCK; ++i) wide[i] = (1ull << 32) + (unsigned long long)i + 1;  // the 64-bit sum carries
      for (const auto& in : {zeros, last, wide})
        CHECK(block_sum_of(block_tag, in) == std::accumulate(in.begin(), in.end(), 0ull));
    };
    check_block_sum(std::integral_constant<int, 256>());
    check_block_sum(std::integral_constant<int, 1024>());

    for (int at : {0, 63}) {  // the minimum at either end of the wavefront
      std::vector<unsigned> in(64);
      for (int i = 0; i < 64; ++i) in[i] = 1000u + (unsigned)((i * 37) % 64);
      in[at] = 3;
      auto d_in = upload(in);
      hip::device_array_t<unsigned> d_out(64);
      wave_min_probe<<<1, 64, 0, ctx.stream()>>>(d_in.data(), d_out.data());
      ctx.synchronize();
      CHECK(d_out.to_host() == std::vector<unsigned>(64, *std::min_element(in.begin(), in.end())));
    }

    auto check_prefix_owner = [&](const std::vector<int>& lengths) {
      std::vector<int> pre(lengths.size());
      std::partial_sum(lengths.begin(), lengths.end(), pre.begin());
      const int cnt = (int)pre.size(), total = pre.back();
      auto d_pre = upload(pre);
      hip::device_array_t<int> d_out(total);
      prefix_owner_probe<<<1, 64, 0, ctx.stream()>>>(d_pre.data(), cnt, total, d_out.data());
      ctx.synchronize();
      std::vector<int> want(total);
      for (int t = 0; t < total; ++t)
        want[t] = (int)(std::upper_bound(pre.begin(), pre.end(), t) - pre.begin());  // smallest i: pre[i] > t
      CHECK(d_out.to_host() == want);
    };
    std::vector<int> lengths = {0, 0, 3, 0, 1, 0};  // leading, interior and trailing empty owners
    lengths.resize(256, 0);
    check_prefix_owner(lengths);
    check_prefix_owner({5});  // a single owner

    hip::device_array_t<int> big_n(1), big(2 * 8);
    big_n.zero();
    big.zero();
    const int rows[3][2] = {{7, 4097}, {9, 8192}, {11, 4096}};  // 2, 2 and 1 segments of 4096
    for (const auto& r : rows)
      push_big_probe<<<1, 64, 0, ctx.stream()>>>(big_n.data(), reinterpret_cast<int2*>(big.data()), r[0], r[1]);
    ctx.synchronize();
    CHECK(big_n.to_host()[0] == 5);
    auto pairs = big.to_host();
    pairs.resize(2 * 5);
    CHECK((pairs == std::vector<int>{7, 0, 7, 1, 9, 0, 9, 1, 11, 0}));
  }

  // ---- the generation queue shared by the kcore / color kernels, each piece against a host loop -----
  {
    // append: 128 vertices with row lengths 1..5, a tail that starts at 7, canaries behind the slots
    std::vector<int> ap(129, 0);
    for (int v = 0; v < 128; ++v) ap[v + 1] = ap[v] + v % 5 + 1;
    auto d_ap = upload(ap);
    const int start = 7, canary = -7;
    auto check_append = [&](auto narrow_tag, const std::vector<int>& ready, int short_by) {
      std::vector<int> want;
      unsigned long long want_degsum = 0;
      for (int v = 0; v < 128; ++v)
        if (ready[v]) {
          want.push_back(v);
          want_degsum += (unsigned long long)(ap[v + 1] - ap[v]);
        }
      const int final_tail = start + (int)want.size(), n = final_tail - short_by;
      auto d_ready = upload(ready);
      auto d_queue = upload(std::vector<int>(final_tail + 8, canary));
      auto d_tail = upload(std::vector<int>{start});
      auto d_degsum = upload(std::vector<unsigned long long>{0});
      queue_append_probe<decltype(narrow_tag)::value><<<1, 128, 0, ctx.stream()>>>(
          d_ready.data(), d_ap.data(), d_queue.data(), n, d_tail.data(), d_degsum.data());
      ctx.synchronize();
      CHECK(d_tail.to_host()[0] == final_tail);
      CHECK(d_degsum.to_host()[0] == want_degsum);
      const auto q = d_queue.to_host();
      bool untouched = true;
      for (int i = 0; i < (int)q.size(); ++i)
        untouched = untouched && (q[i] == canary || (i >= start && i < n));
      CHECK(untouched);  // nothing before the tail, nothing at or beyond n
      std::vector<int> got(q.begin() + start, q.begin() + n);
      std::sort(got.begin(), got.end());
      CHECK(std::adjacent_find(got.begin(), got.end()) == got.end());               // each once
      CHECK(std::includes(want.begin(), want.end(), got.begin(), got.end()));        // only ready vertices
      CHECK((int)got.size() == (int)want.size() - short_by && got.front() != canary);  // every slot below n
    };
    std::vector<int> few(128, 0), all(128, 1);
    few[5] = few[17] = few[63] = 1;  // wavefront 1 has no ready lane
    for (const auto& ready : {few, all})
      for (int short_by : {0, 2}) {
        check_append(std::false_type(), ready, short_by);
        check_append(std::true_type(), ready, short_by);
      }

    // walk: owner i holds vertex order[i]; returns {entries, dead calls, rows on the big list}
    auto check_walk = [&](const std::vector<int>& owner_lengths, int big_row) {
      const std::vector<int> order = {4, 2, 0, 3, 1};
      std::vector<int> lengths(5), wap(6, 0);
      for (int i = 0; i < 5; ++i) lengths[order[i]] = owner_lengths[i];
      for (int v = 0; v < 5; ++v) wap[v + 1] = wap[v] + lengths[v];
      std::vector<int> want_visits(wap[5] + 1, 0), want_owners(wap[5] + 1, -1), want_big;
      int want_entries = 0;
      for (int i = 0; i < 5; ++i) {
        if (owner_lengths[i] > big_row) {
          want_big.push_back(order[i]);
          continue;
        }
        want_entries += owner_lengths[i];
        for (int e = wap[order[i]]; e < wap[order[i] + 1]; ++e) {
          want_visits[e] = 1;
          want_owners[e] = i;
        }
      }
      auto d_wap = upload(wap);
      auto d_queue = upload(order);
      auto d_visits = upload(std::vector<int>(wap[5] + 1, 0));
      auto d_owners = upload(std::vector<int>(wap[5] + 1, -1));
      auto d_misc = upload(std::vector<int>{0, 0, -1});  // big_n, dead calls, entries
      hip::device_array_t<int> d_big(5);
      queue_walk_probe<<<1, 256, 0, ctx.stream()>>>(d_wap.data(), d_queue.data(), 5, big_row, d_big.data(), d_misc.data(),
                                                   d_visits.data(), d_owners.data(), d_misc.data() + 1,
                                                   d_misc.data() + 2);
      ctx.synchronize();
      const auto misc = d_misc.to_host();
      auto on_big = d_big.to_host();
      on_big.resize(std::min(misc[0], 5));
      CHECK(d_visits.to_host() == want_visits && d_owners.to_host() == want_owners);
      CHECK(misc[2] == want_entries && on_big == want_big);
      CHECK(misc[1] == (want_entries + 255) / 256 * 256 - want_entries);
      return std::vector<int>{misc[2], misc[1], misc[0]};
    };
    // 365 entries: one BLOCK boundary crossed, not a multiple of 64
    CHECK((check_walk({0, 1, 300, 0, 64}, INT_MAX) == std::vector<int>{365, 2 * 256 - 365, 0}));
    CHECK((check_walk({0, 0, 0, 0, 0}, INT_MAX) == std::vector<int>{0, 0, 0}));
    CHECK((check_walk({0, 1, 300, 0, 64}, 100) == std::vector<int>{65, 256 - 65, 1}));  // the long row: listed once, not walked

    // narrow loop: generations {0}, {1}, {2}, {3} of 3, 5, 100 and 7 entries; the third is too large
    {
      const std::vector<int> cap = {0, 3, 8, 108, 115};
      auto d_cap = upload(cap);
      auto d_queue = upload(std::vector<int>{0, -1, -1, -1});
      hip::kernels::queue_counters_t c{};
      c.tail = 1;
      c.degsum = 3;
      auto d_ctr = upload(std::vector<hip::kernels::queue_counters_t>{c});
      hip::device_array_t<hip::kernels::narrow_result_t> d_out(1);
      narrow_generations_probe<<<1, 1024, 0, ctx.stream()>>>(d_ctr.data(), d_cap.data(), d_queue.data(), 4, 50ull,
                                                            d_out.data());
      ctx.synchronize();
      const auto r = d_out.to_host()[0];
      CHECK(r.generations == 2 && r.head == 2 && r.tail == 3);  // stopped with the third pending
      CHECK(r.degsum == 100 && r.walked == 3 + 5);
      CHECK((d_queue.to_host() == std::vector<int>{0, 1, 2, -1}));
    }
  }

  // ---- unsupported variants throw (reference advance.hxx:121-127) ---------------------------
  {
    frontier_t a, b;
    a.push_back(1);
    hip::device_array_t<edge_t> seg;
    auto op = [] __host__ __device__(vertex_t const&, vertex_t const&, edge_t const&, weight_t const&) -> bool { return true; };
    bool threw = false;
    try {
      operators::advance::execute<lbt::block_mapped, operators::advance_direction_t::optimized,
                                  operators::advance_io_type_t::vertices,
                                  operators::advance_io_type_t::vertices>(G, op, &a, &b, seg, *mc);
    } catch (error::exception_t&) { threw = true; }
    CHECK(threw);
    // pull needs in-edges: a graph marked directed (and without a csc view) is refused
    auto Gd = G;
    Gd.properties.directed = true;
    threw = false;
    try {
      operators::advance::execute<lbt::block_mapped, operators::advance_direction_t::backward,
                                  operators::advance_io_type_t::vertices,
                                  operators::advance_io_type_t::vertices>(Gd, op, &a, &b, seg, *mc);
    } catch (error::exception_t&) { threw = true; }
    CHECK(threw);
    gcuda::multi_context_t two(std::vector<int>{0, 0});
    threw = false;
    try {
      operators::advance::execute<lbt::block_mapped, operators::advance_direction_t::forward,
                                  operators::advance_io_type_t::vertices,
                                  operators::advance_io_type_t::vertices>(G, op, &a, &b, seg, two);
    } catch (error::exception_t&) { threw = true; }
    CHECK(threw);
  }

  // ---- batch: independent runs on host threads, each with its own context ---------------------
  {
    std::vector<int> degsum(12, 0);
    auto job = [&](std::size_t j) -> float {
      auto my = std::make_shared<gcuda::multi_context_t>(0);
      frontier_t fin, fout;
      fin.push_back((int)j);
      hip::device_array_t<edge_t> seg;
      auto op = [] __host__ __device__(vertex_t const&, vertex_t const&, edge_t const&, weight_t const&) -> bool { return true; };
      operators::advance::execute<lbt::block_mapped, operators::advance_direction_t::forward,
                                  operators::advance_io_type_t::vertices,
                                  operators::advance_io_type_t::vertices>(G, op, &fin, &fout, seg, *my);
      degsum[j] = (int)fout.get_number_of_elements();
      return 1.0f;
    };
    float total = 0;
    operators::batch::execute(job, degsum.size(), &total);
    CHECK(total == (float)degsum.size());
    for (std::size_t j = 0; j < degsum.size(); ++j) CHECK(degsum[j] == hg.ap[j + 1] - hg.ap[j]);
  }

  if (dump) {
    dump_array("failures", std::vector<int>{failures}, true);
    std::fprintf(dump, "}\n");
    std::fclose(dump);
  }
  std::printf(failures ? "engine_tests: %d FAILURES\n" : "engine_tests: all passed\n", failures);
  return failures ? 1 : 0;
}

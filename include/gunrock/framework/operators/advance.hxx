/**
 * @file advance.hxx
 * @brief operators::advance::execute -- neighbour expansion of a frontier.
 *
 * API of reference framework/operators/advance/advance.hxx:91-129 (frontier
 * overload) and :192-221 (enactor overload): template arguments <load balance,
 * direction, input type, output type>, functor bool(src, dst, edge, weight),
 * buffers swapped afterwards unless output_type == none or swap_buffers == false.
 * Unsupported combinations throw error::exception_t, like the reference.
 *
 * Host-side structure (per call, all on the context's stream):
 *   1. size the output (detail::open_frame): skipped when n_in * max_degree(G) already fits the
 *      output frontier; otherwise one degree-sum kernel + a pinned read-back (the
 *      reference does this reduction on EVERY call: advance/helpers.hxx:112-146);
 *   2. the expansion kernel(s) of the chosen schedule;
 *   3. ONE hand-off of the counters (detail::close_frame, hip/hand_off.hxx), which the host waits
 *      for (operators are synchronous, like block_mapped.hxx:204) and which leaves them zero.
 * No allocation happens in the steady state (the reference allocates a device
 * cursor per call, block_mapped.hxx:200).
 */
#pragma once

#include <gunrock/framework/operators/by_destination.hxx>
#include <gunrock/framework/operators/configs.hxx>
#include <gunrock/hip/context.hxx>
#include <gunrock/hip/hand_off.hxx>
#include <gunrock/hip/kernels/advance_kernels.hxx>
#include <gunrock/hip/primitives.hxx>

#include <mutex>
#include <type_traits>

/// Compile-time override of the schedule hard-coded by a client header, e.g.
/// -DGRX_ADVANCE_LB_OVERRIDE=bucketing to run the unchanged sssp.hxx (which
/// spells block_mapped, algorithms/sssp.hxx:139) with degree bucketing.
#ifdef GRX_ADVANCE_LB_OVERRIDE
#define GRX_LB_EFFECTIVE(lb) (::gunrock::operators::load_balance_t::GRX_ADVANCE_LB_OVERRIDE)
#else
#define GRX_LB_EFFECTIVE(lb) (lb)
#endif

namespace gunrock {
namespace operators {
namespace advance {

namespace detail {

namespace k = ::gunrock::hip::kernels;

template <typename graph_t>
unsigned long long max_degree(graph_t& G, gcuda::standard_context_t& ctx) {
  if (G.properties.max_degree)  // the view's builder knows it
    return G.properties.max_degree;
  auto& ws = ctx.workspace();
  const void* key = (const void*)G.get_row_offsets();
  const std::size_t n = (std::size_t)G.get_number_of_vertices();
  const std::size_t m = (std::size_t)G.get_number_of_edges();
  if (auto* f = ws.find_graph(key, n, m))
    return f->max_degree;
  unsigned long long* counters = ws.counters();
  if (n) {
    k::max_degree_kernel<<<hip::grid_for(n, k::ADV_BLOCK, 1024), k::ADV_BLOCK, 0, ctx.stream()>>>(
        G, counters);
    GRX_HIP_CHECK(hipGetLastError());
  }
  unsigned long long md = hip::fetch_counters(ctx)[k::C_MAXDEG];
  if (std::getenv("GRX_DEBUG"))
    std::fprintf(stderr, "[grx] max_degree(%zu vertices) = %llu (seq %llu)\n", n, md,
                 ws.mirror()[gcuda::workspace_t::sequence_slot]);
  gcuda::workspace_t::graph_facts_t facts{key, n, md, m};
  return ws.remember_graph(facts)->max_degree;
}

/// Sum of degrees of the valid input slots (64-bit).
template <advance_io_type_t input_type, typename graph_t, typename vertex_t>
unsigned long long degree_sum(graph_t& G, const vertex_t* input, std::size_t n_in,
                              gcuda::standard_context_t& ctx) {
  if (input_type == advance_io_type_t::graph)
    return (unsigned long long)G.get_number_of_edges();
  k::degree_sum_kernel<input_type><<<hip::grid_for(n_in, k::ADV_BLOCK, 1024), k::ADV_BLOCK, 0,
                                     ctx.stream()>>>(G, input, n_in, ctx.workspace().counters());
  GRX_HIP_CHECK(hipGetLastError());
  return hip::fetch_counters(ctx)[k::C_WORK];
}

/// segments[0..n_in] = exclusive scan of the input slots' degrees; returns the total.
/// (reference advance/helpers.hxx:38-96, compute_output_offsets)
template <advance_io_type_t input_type, typename graph_t, typename vertex_t, typename work_tiles_t>
unsigned long long scan_degrees(graph_t& G, const vertex_t* input, std::size_t n_in,
                                work_tiles_t& segments, gcuda::standard_context_t& context) {
  using edge_t = typename graph_t::edge_type;
  if (segments.size() < n_in + 1)
    segments.resize(n_in + 1);
  edge_t* seg = segments.data();
  k::slot_degree_kernel<input_type><<<hip::grid_for(n_in + 1, k::ADV_BLOCK, 4096),
                                      k::ADV_BLOCK, 0, context.stream()>>>(G, input, n_in, seg);
  GRX_HIP_CHECK(hipGetLastError());
  std::size_t bytes = hip::exclusive_sum_temp_bytes(seg, seg, edge_t(0), n_in + 1);
  void* temp = context.workspace().scratch(bytes);
  hip::exclusive_sum(temp, bytes, seg, seg, edge_t(0), n_in + 1, context.stream());
  auto& ws = context.workspace();
  edge_t* landing = reinterpret_cast<edge_t*>(ws.mirror() + 24);
  GRX_HIP_CHECK(hipMemcpyAsync(landing, seg + n_in, sizeof(edge_t), hipMemcpyDeviceToHost,
                               context.stream()));
  context.synchronize();
  return (unsigned long long)*landing;
}

/// How an ascending frontier is dealt across the tiles of the wide-level kernels (advance_kernels.hxx):
/// across the tiles workgroup-major by the settled kernel, in groups of 16 slots by the fused kernel
/// (0 = consecutive slots, what every other frontier gets).
constexpr int DEALT_SETTLED = 2, DEALT_FUSED = 1;

inline unsigned long long saturating_mul(unsigned long long a, unsigned long long b) {
  if (a == 0 || b == 0)
    return 0;
  if (a > ~0ull / b)
    return ~0ull;
  return a * b;
}

/**
 * @brief Make sure `output` can take the result.  Returns false when the
 * operator has nothing to do (no work), with the output already set empty.
 * `total` receives the exact work size when it had to be computed (else ~0).
 */
template <advance_io_type_t input_type, typename graph_t, typename frontier_t>
bool size_output(graph_t& G, frontier_t& input, frontier_t& output, std::size_t n_in, bool exact,
                 unsigned long long& total, gcuda::standard_context_t& ctx) {
  total = ~0ull;
  unsigned long long bound = saturating_mul(n_in, max_degree(G, ctx));
  if (input_type != advance_io_type_t::graph && input.work_hint() < bound)
    bound = input.work_hint();  // left by the operator that produced this frontier
  if (input_type == advance_io_type_t::graph)
    bound = (unsigned long long)G.get_number_of_edges();
  if (!exact && bound <= output.get_capacity())
    return true;
  total = degree_sum<input_type>(G, input.data(), n_in, ctx);
  if (total == 0) {
    output.set_number_of_elements(0);
    return false;
  }
  if (output.get_capacity() < total)
    output.reserve(total);
  return true;
}

template <typename frontier_t>
void finish_output(frontier_t& output, bool holes, unsigned long long total,
                   gcuda::standard_context_t& ctx) {
  unsigned long long* m = hip::fetch_counters(ctx);
  ctx.kernel_clock().collect();
  if (std::getenv("GRX_DEBUG"))
    std::fprintf(stderr, "[grx] advance done: out %llu chunks %llu next_work %llu\n", m[k::C_OUT],
                 m[k::C_CHUNKS], m[k::C_NEXT_WORK]);
#ifdef GRX_TILE_TIMING
  if (std::getenv("GRX_DEBUG") && m[30])
    std::fprintf(stderr,
                 "[grx] tile timing (us, mean per workgroup of %llu): stage %.1f edges %.1f drain %.1f "
                 "total %.1f max-total %.1f | tiles/wg %.2f iters/wg %.2f\n",
                 m[30], m[24] / 100.0 / m[30], m[25] / 100.0 / m[30], m[29] / 100.0 / m[30],
                 m[28] / 100.0 / m[30], m[7] / 100.0, (double)m[27] / m[30], (double)m[26] / m[30]);
#endif
  error::throw_if_exception(m[k::C_OVERFLOW] != 0,
                            "advance: output frontier capacity exceeded");
  output.set_number_of_elements(holes ? (std::size_t)total : (std::size_t)m[k::C_OUT]);
  if (!holes)
    output.set_work_hint(m[k::C_NEXT_WORK]);
}

// ---------------------------------------------------------------------------
// The call frame every schedule shares: open_frame() before its kernels, close_frame() behind them.
// ---------------------------------------------------------------------------

/// How open_frame() makes room in the output frontier.  frame_t::holes follows from it: the holes
/// layout is honoured by `bounded` and `scanned` only (`packed` is `bounded` for the schedules that
/// cannot place holes; the dispatcher sends their holes calls to merge_path).
enum class sizing_t {
  packed,     ///< a bound (size_output); the schedule has no holes layout (warp_mapped, bucketing)
  bounded,    ///< a bound, or the exact degree sum under the holes layout (block_mapped, thread_mapped)
  scanned,    ///< exact, by the degree scan left in `segments` (merge_path; thread_mapped's holes layout)
  candidates  ///< at most one output slot per input slot (pull)
};

template <typename vertex_t>
struct frame_t {
  std::size_t n_in = 0;             ///< input slots
  bool holes = false;               ///< one output slot per edge, invalid where the functor said no
  unsigned long long total = ~0ull; ///< the exact work size where sizing computed it
  vertex_t* out_ptr = nullptr;      ///< the output frontier's slots and their number (none: null, 0)
  std::size_t capacity = 0;
  unsigned long long* counters = nullptr;
};

/// The prologue.  Returns false when there is nothing to do, with the output already set empty.
template <advance_io_type_t input_type,
          advance_io_type_t output_type,
          typename graph_t,
          typename frontier_t,
          typename work_tiles_t = std::nullptr_t>
bool open_frame(frame_t<typename graph_t::vertex_type>& f, sizing_t sizing, graph_t& G, frontier_t& input,
                frontier_t& output, gcuda::standard_context_t& ctx, work_tiles_t segments = nullptr) {
  constexpr bool has_out = (output_type != advance_io_type_t::none);
  auto nothing_to_do = [&] {
    if constexpr (has_out)
      output.set_number_of_elements(0);
    return false;
  };
  f.n_in = (input_type == advance_io_type_t::graph) ? (std::size_t)G.get_number_of_vertices()
                                                    : input.get_number_of_elements();
  if (f.n_in == 0)
    return nothing_to_do();
  f.holes = has_out && ctx.options().holes_layout &&
            (sizing == sizing_t::bounded || sizing == sizing_t::scanned);
  if (sizing == sizing_t::scanned) {
    error::throw_if_exception(!std::is_pointer<work_tiles_t>::value, "advance: a degree scan needs `segments`");
    if constexpr (std::is_pointer<work_tiles_t>::value)
      f.total = scan_degrees<input_type>(G, input.data(), f.n_in, *segments, ctx);
    if (f.total == 0)
      return nothing_to_do();
    if (has_out && output.get_capacity() < f.total)
      output.reserve(f.total);
  } else if (sizing == sizing_t::candidates) {
    if (has_out && output.get_capacity() < f.n_in)
      output.reserve(f.n_in);
  } else if (has_out) {
    if (!size_output<input_type>(G, input, output, f.n_in, f.holes, f.total, ctx))
      return false;
  }
  if constexpr (has_out) {
    f.out_ptr = output.data();
    f.capacity = output.get_capacity();
  }
  f.counters = ctx.workspace().counters();
  return true;
}

/// The epilogue: close the kernel-time interval and hand the counters over, which waits for the
/// kernels and leaves the counters clean.  `may_defer`: a call without an output only enqueues
/// when the client set defer_sync_of_none_output -- the operator that follows fetches the counters
/// and stops the clock.
template <advance_io_type_t output_type, typename frontier_t, typename vertex_t>
void close_frame(hip::clocked_t& clock, frontier_t& output, const frame_t<vertex_t>& f,
                 gcuda::standard_context_t& ctx, bool may_defer = false) {
  constexpr bool has_out = (output_type != advance_io_type_t::none);
  GRX_HIP_CHECK(hipGetLastError());
  if (!has_out && may_defer && ctx.options().defer_sync_of_none_output)
    return;
  clock.stop();
  if constexpr (has_out) {
    finish_output(output, f.holes, f.total, ctx);
  } else {
    hip::fetch_counters(ctx);
    ctx.kernel_clock().collect();
  }
}

/// launch(std::true_type / std::false_type): the run-time layout flag as a template argument.
template <typename launch_t>
void with_holes(bool holes, launch_t&& launch) {
  if (holes)
    launch(std::true_type());
  else
    launch(std::false_type());
}

/// What the hub kernels of a call share: the device chunk queue and the two thresholds.
template <typename vertex_t, typename edge_t>
struct hub_plan_t {
  k::chunk_t<vertex_t, edge_t>* chunks;
  unsigned long long chunk_capacity;
  unsigned hub_threshold, chunk_edges;
};

/// The chunk queue is sized for every hub of this call: a list of d edges makes at most
/// d / chunk_edges + 1 chunks, and only lists of >= hub_threshold edges make any.
template <typename vertex_t, typename edge_t, typename graph_t>
hub_plan_t<vertex_t, edge_t> plan_hubs(graph_t& G, std::size_t n_in, unsigned long long work_bound,
                                       gcuda::standard_context_t& ctx) {
  const unsigned chunk_edges = ctx.options().chunk_edges ? ctx.options().chunk_edges : 1024u;
  const unsigned hub = ctx.options().hub_threshold ? ctx.options().hub_threshold : 1u;
  unsigned long long hubs = n_in;
  if (work_bound != ~0ull) {
    if (work_bound / hub < hubs)
      hubs = work_bound / hub;
  } else {
    work_bound = (unsigned long long)G.get_number_of_edges() + (unsigned long long)n_in * hub;
  }
  unsigned long long capacity = work_bound / chunk_edges + hubs + 1024;
  if (ctx.options().chunk_queue_limit && capacity > ctx.options().chunk_queue_limit)
    capacity = ctx.options().chunk_queue_limit;
  auto* chunks = reinterpret_cast<k::chunk_t<vertex_t, edge_t>*>(
      ctx.workspace().queue(capacity * sizeof(k::chunk_t<vertex_t, edge_t>)));
  return {chunks, capacity, ctx.options().hub_threshold, chunk_edges};
}

/// The edges a call expands at most: its exact total where sizing computed one, else the work
/// hint its input came with.
template <advance_io_type_t input_type, typename graph_t, typename frontier_t>
unsigned long long work_bound_of(graph_t& G, frontier_t& input, unsigned long long total) {
  if (total != ~0ull)
    return total;
  return (input_type == advance_io_type_t::graph) ? (unsigned long long)G.get_number_of_edges()
                                                  : input.work_hint();
}

/// Hub pre-pass of the wide-level forms (advance_kernels.hxx: classify_hubs_kernel).  Returns the
/// scratch it fills: [8 claim cursors, one 128-B line each | hub mask, one bit per input slot].
template <advance_io_type_t input_type, typename graph_t, typename vertex_t, typename edge_t>
unsigned long long* classify_hubs(graph_t& G, const vertex_t* input, std::size_t n_in,
                                  const unsigned long long* n_in_device,
                                  const hub_plan_t<vertex_t, edge_t>& hubs, gcuda::standard_context_t& ctx) {
  auto* cursors = reinterpret_cast<unsigned long long*>(ctx.workspace().scratch(
      (8 * k::CLAIM_LINE + (n_in + 63) / 64) * sizeof(unsigned long long)));
  k::classify_hubs_kernel<input_type>
      <<<hip::grid_for(n_in, k::CLASSIFY_TILE, (unsigned)ctx.compute_units() * 8u), k::ADV_BLOCK, 0,
         ctx.stream()>>>(G, input, n_in, n_in_device, hubs.chunks, hubs.chunk_capacity, hubs.hub_threshold,
                         hubs.chunk_edges, cursors + 8 * k::CLAIM_LINE, cursors, ctx.workspace().counters());
  return cursors;
}

/// The dynamic-LDS opt-in of ONE kernel instantiation (dynamic LDS beyond 64 KB needs one per device):
/// made once, for all the room its static LDS leaves of a CU's 160 KB, when the static size is first
/// asked for.  Handles are shared between host threads: one lock around the look-up-and-set.
struct lds_opt_in_t {
  static constexpr std::size_t cu_lds = 160u << 10;
  std::mutex lock;
  std::size_t static_bytes[64] = {};  // by device ordinal
  bool known[64] = {};
  /// Do `lds` bytes of dynamic LDS fit beside `kernel`'s static LDS?
  bool fits(const void* kernel, std::size_t lds, gcuda::standard_context_t& ctx) {
    const int device = ctx.ordinal() & 63;
    std::lock_guard<std::mutex> guard(lock);
    if (!known[device]) {
      hipFuncAttributes fa;
      GRX_HIP_CHECK(hipFuncGetAttributes(&fa, kernel));
      GRX_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)(cu_lds - fa.sharedSizeBytes)));
      static_bytes[device] = fa.sharedSizeBytes;
      known[device] = true;
    }
    return static_bytes[device] + lds <= cu_lds;
  }
};

/**
 * @brief The wide-level form of a client that named its settled destinations (operators/settled.hxx):
 * hub pre-pass, then one 1024-thread workgroup per CU with the client's image in its LDS
 * (advance_kernels.hxx: expand_settled_kernel).  `n_in_device` (nullable): the frontier length is
 * read on the device, at most `n_in`.  Only enqueues.  Returns false, with nothing enqueued, when the
 * kernel's static LDS + the image do not fit the CU (a wide edge_t makes the static part larger).
 * `op` is the caller's copy: a hint without an image is told so for whatever the caller runs next.
 */
template <advance_io_type_t input_type,
          advance_io_type_t output_type,
          typename graph_t,
          typename operator_t,
          typename vertex_t,
          typename edge_t>
bool enqueue_settled(graph_t& G, operator_t& op, const vertex_t* input, std::size_t n_in,
                     const unsigned long long* n_in_device, const hub_plan_t<vertex_t, edge_t>& hubs,
                     vertex_t* output, std::size_t capacity, int dealt, gcuda::standard_context_t& ctx) {
  auto kernel = k::expand_settled_kernel<input_type, output_type, graph_t, operator_t, vertex_t, edge_t>;
  if (!op.settled.bits)  // a predicate only: no image to keep in LDS
    op.settled.limit = 0;
  const std::size_t lds = op.settled.limit > 0 ? op.lds_bytes() : 16;
  static lds_opt_in_t opt_in;  // of this instantiation of the kernel
  if (!opt_in.fits(reinterpret_cast<const void*>(kernel), lds, ctx))
    return false;
  unsigned long long* cursors = classify_hubs<input_type>(G, input, n_in, n_in_device, hubs, ctx);
  kernel<<<(unsigned)ctx.compute_units(), k::SET_BLOCK, lds, ctx.stream()>>>(
      G, op, input, n_in, output, capacity, ctx.workspace().counters(), hubs.chunks, hubs.chunk_capacity,
      cursors + 8 * k::CLAIM_LINE, cursors, n_in_device, dealt);
  GRX_HIP_CHECK(hipGetLastError());
  return true;
}

}  // namespace detail

// ===========================================================================
// block_mapped (and work_stealing = the same kernel with dynamic tile claims)
// ===========================================================================
namespace block_mapped {

template <advance_direction_t direction,
          advance_io_type_t input_type,
          advance_io_type_t output_type,
          bool dynamic_tiles = false,
          typename graph_t,
          typename operator_t,
          typename frontier_t>
void execute(graph_t& G,
             operator_t op,
             frontier_t& input,
             frontier_t& output,
             gcuda::standard_context_t& context) {
  namespace k = detail::k;
  using vertex_t = typename graph_t::vertex_type;
  using edge_t = typename graph_t::edge_type;
  constexpr bool has_out = (output_type != advance_io_type_t::none);

  detail::frame_t<vertex_t> f;
  if (!detail::open_frame<input_type, output_type>(f, detail::sizing_t::bounded, G, input, output, context))
    return;
  if constexpr (!has_out)  // kept: a view built without properties.max_degree (the C++ surface) has it
    (void)detail::max_degree(G, context);  // reduced and remembered by its first call, output or not
  const unsigned long long work_bound = detail::work_bound_of<input_type>(G, input, f.total);
  const auto hubs = detail::plan_hubs<vertex_t, edge_t>(G, f.n_in, work_bound, context);
  const unsigned persistent = (unsigned)context.compute_units() * context.options().tile_blocks_per_cu;
  const std::size_t n_tiles = (f.n_in + k::ADV_BLOCK - 1) / k::ADV_BLOCK;
  const unsigned grid = (unsigned)(n_tiles < persistent ? n_tiles : persistent);
  const bool ascending = input_type == advance_io_type_t::vertices && input.ascending();

  hip::clocked_t clock(context);
  // wide frontiers: hub pre-pass + ONE kernel that expands tiles and then claims hub chunks
  // dynamically (advance_kernels.hxx: classify_hubs_kernel / expand_fused_kernel)
  const std::size_t fused_from = context.options().fused_min_slots;
  bool use_settled = false;
  if constexpr (settled_traits<operator_t>::value)
    use_settled = ((op.settled.bits && op.settled.limit > 0) || operator_t::has_predicate) &&
                  context.options().settled_filter && work_bound != ~0ull &&
                  work_bound >= context.options().settled_min_work;
  if (!f.holes && !dynamic_tiles && ((fused_from && f.n_in >= fused_from) || use_settled)) {
    bool expanded = false;
    if constexpr (settled_traits<operator_t>::value) {
      if (use_settled)  // where the image does not fit, the fused form calls the functor for every edge
        expanded = detail::enqueue_settled<input_type, output_type>(
            G, op, input.data(), f.n_in, (const unsigned long long*)nullptr, hubs, f.out_ptr, f.capacity,
            ascending ? detail::DEALT_SETTLED : 0, context);
    }
    if (!expanded) {
      unsigned long long* cursors = detail::classify_hubs<input_type>(
          G, input.data(), f.n_in, (const unsigned long long*)nullptr, hubs, context);
      const unsigned fgrid = (unsigned)context.compute_units() * context.options().fused_blocks_per_cu;
      k::expand_fused_kernel<input_type, output_type><<<fgrid, k::ADV_BLOCK, 0, context.stream()>>>(
          G, op, input.data(), f.n_in, nullptr, f.out_ptr, f.capacity, f.counters, hubs.chunks,
          hubs.chunk_capacity, cursors + 8 * k::CLAIM_LINE, cursors, ascending ? detail::DEALT_FUSED : 0);
    }
  } else {
    detail::with_holes(f.holes, [&](auto holes) {
      k::block_mapped_kernel<decltype(holes)::value, dynamic_tiles, input_type, output_type>
          <<<grid, k::ADV_BLOCK, 0, context.stream()>>>(G, op, input.data(), f.n_in, f.out_ptr, f.capacity,
                                                        f.counters, hubs.chunks, hubs.chunk_capacity,
                                                        hubs.hub_threshold, hubs.chunk_edges, nullptr);
    });
    // packed output: the hub chunks the tiles queued.  Whether any were queued is the DEVICE's
    // knowledge: a remembered max degree (keyed by address) must never decide if they are expanded
    if (!f.holes)
      k::chunk_kernel<output_type>
          <<<(unsigned)context.compute_units() * context.options().chunk_blocks_per_cu, k::ADV_BLOCK, 0,
             context.stream()>>>(G, op, hubs.chunks, hubs.chunk_capacity, f.out_ptr, f.capacity, f.counters);
  }
  detail::close_frame<output_type>(clock, output, f, context, /*may_defer=*/true);
#ifdef GRX_SETTLED_STATS
  if (use_settled) {
    const unsigned long long* m = context.workspace().mirror();
    std::fprintf(stderr, "[settled] slots %zu work %llu: rounds %llu, predicate tests %llu, functor calls %llu "
                 "carrying %llu edges\n", f.n_in, work_bound, m[14], m[13], m[10], m[11]);
  }
#endif
}

/**
 * @brief Enqueue-only form for fused pipelines (vertex-partitioned supersteps): packed output,
 * frontier length read from DEVICE memory (`n_in_device`, at most `n_in_bound`), nothing fetched,
 * nothing awaited.  The caller reads counters[C_OUT] / the counters' hand-off later.
 */
template <typename graph_t, typename operator_t, typename vertex_t>
void enqueue_packed(graph_t& G,
                    operator_t op,
                    const vertex_t* input,
                    std::size_t n_in_bound,
                    const unsigned long long* n_in_device,
                    unsigned long long work_bound,
                    vertex_t* output,
                    std::size_t capacity,
                    gcuda::standard_context_t& context) {
  namespace k = detail::k;
  using edge_t = typename graph_t::edge_type;
  constexpr advance_io_type_t vin = advance_io_type_t::vertices;
  if (n_in_bound == 0)
    return;
  const auto hubs = detail::plan_hubs<vertex_t, edge_t>(G, n_in_bound, work_bound, context);
  unsigned long long* counters = context.workspace().counters();
  const std::size_t n_tiles = (n_in_bound + k::ADV_BLOCK - 1) / k::ADV_BLOCK;
  const unsigned persistent = (unsigned)context.compute_units() * context.options().tile_blocks_per_cu;
  const unsigned grid = (unsigned)(n_tiles < persistent ? n_tiles : persistent);
  k::block_mapped_kernel<false, false, vin, vin><<<grid, k::ADV_BLOCK, 0, context.stream()>>>(
      G, op, input, n_in_bound, output, capacity, counters, hubs.chunks, hubs.chunk_capacity,
      hubs.hub_threshold, hubs.chunk_edges, n_in_device);
  k::chunk_kernel<vin><<<(unsigned)context.compute_units() * context.options().chunk_blocks_per_cu,
                           k::ADV_BLOCK, 0, context.stream()>>>(G, op, hubs.chunks, hubs.chunk_capacity,
                                                                output, capacity, counters);
  GRX_HIP_CHECK(hipGetLastError());
}

/**
 * @brief enqueue_packed for a WIDE frontier of a client that named its settled destinations
 * (operators/settled.hxx): detail::enqueue_settled with the frontier length read on the device,
 * nothing fetched, nothing awaited.  Returns false (nothing enqueued) when the kernel's LDS image
 * does not fit this device: the caller falls back to enqueue_packed.
 */
template <typename graph_t, typename operator_t, typename vertex_t>
bool enqueue_packed_settled(graph_t& G,
                            operator_t op,
                            const vertex_t* input,
                            std::size_t n_in_bound,
                            const unsigned long long* n_in_device,
                            unsigned long long work_bound,
                            vertex_t* output,
                            std::size_t capacity,
                            gcuda::standard_context_t& context) {
  using edge_t = typename graph_t::edge_type;
  constexpr advance_io_type_t vin = advance_io_type_t::vertices;
  static_assert(settled_traits<operator_t>::value, "enqueue_packed_settled takes a hinted functor");
  if (n_in_bound == 0)
    return true;
  const auto hubs = detail::plan_hubs<vertex_t, edge_t>(G, n_in_bound, work_bound, context);
  return detail::enqueue_settled<vin, vin>(G, op, input, n_in_bound, n_in_device, hubs, output, capacity, 0,
                                           context);
}

}  // namespace block_mapped

// ===========================================================================
// merge_path: device-wide degree scan + equal shares of edges
// ===========================================================================
namespace merge_path {

template <advance_direction_t direction,
          advance_io_type_t input_type,
          advance_io_type_t output_type,
          typename graph_t,
          typename operator_t,
          typename frontier_t,
          typename work_tiles_t>
void execute(graph_t& G,
             operator_t op,
             frontier_t& input,
             frontier_t& output,
             work_tiles_t& segments,
             gcuda::standard_context_t& context) {
  namespace k = detail::k;
  detail::frame_t<typename graph_t::vertex_type> f;
  if (!detail::open_frame<input_type, output_type>(f, detail::sizing_t::scanned, G, input, output, context,
                                                   &segments))
    return;
  const unsigned grid = hip::grid_for(f.total, k::MP_TILE, (unsigned)context.compute_units() * 8u);
  hip::clocked_t clock(context);
  detail::with_holes(f.holes, [&](auto holes) {
    k::merge_path_kernel<decltype(holes)::value, input_type, output_type>
        <<<grid, k::ADV_BLOCK, 0, context.stream()>>>(G, op, input.data(), f.n_in, segments.data(), f.total,
                                                      f.out_ptr, f.capacity, f.counters);
  });
  detail::close_frame<output_type>(clock, output, f, context);
}

}  // namespace merge_path

// ===========================================================================
// thread_mapped / warp_mapped
// ===========================================================================
namespace thread_mapped {

template <advance_direction_t direction,
          advance_io_type_t input_type,
          advance_io_type_t output_type,
          typename graph_t,
          typename operator_t,
          typename frontier_t,
          typename work_tiles_t>
void execute(graph_t& G,
             operator_t op,
             frontier_t& input,
             frontier_t& output,
             work_tiles_t& segments,
             gcuda::standard_context_t& context) {
  namespace k = detail::k;
  using edge_t = typename graph_t::edge_type;
  constexpr bool has_out = (output_type != advance_io_type_t::none);
  // the holes layout takes its output positions from a degree scan
  const bool scan = has_out && context.options().holes_layout;
  detail::frame_t<typename graph_t::vertex_type> f;
  if (!detail::open_frame<input_type, output_type>(
          f, scan ? detail::sizing_t::scanned : detail::sizing_t::bounded, G, input, output, context, &segments))
    return;
  const edge_t* seg = scan ? segments.data() : nullptr;
  const unsigned grid = hip::grid_for(f.n_in, k::ADV_BLOCK, (unsigned)context.compute_units() * 8u);
  hip::clocked_t clock(context);
  detail::with_holes(f.holes, [&](auto holes) {
    k::thread_mapped_kernel<decltype(holes)::value, input_type, output_type>
        <<<grid, k::ADV_BLOCK, 0, context.stream()>>>(G, op, input.data(), f.n_in, seg, f.out_ptr, f.capacity,
                                                      f.counters);
  });
  detail::close_frame<output_type>(clock, output, f, context);
}

}  // namespace thread_mapped

namespace warp_mapped {

template <advance_direction_t direction,
          advance_io_type_t input_type,
          advance_io_type_t output_type,
          typename graph_t,
          typename operator_t,
          typename frontier_t>
void execute(graph_t& G,
             operator_t op,
             frontier_t& input,
             frontier_t& output,
             gcuda::standard_context_t& context) {
  namespace k = detail::k;
  detail::frame_t<typename graph_t::vertex_type> f;
  if (!detail::open_frame<input_type, output_type>(f, detail::sizing_t::packed, G, input, output, context))
    return;
  const unsigned grid = hip::grid_for(f.n_in, k::ADV_WAVES, (unsigned)context.compute_units() * 8u);
  hip::clocked_t clock(context);
  k::wave_mapped_kernel<input_type, output_type><<<grid, k::ADV_BLOCK, 0, context.stream()>>>(
      G, op, input.data(), f.n_in, f.out_ptr, f.capacity, f.counters);
  detail::close_frame<output_type>(clock, output, f, context);
}

}  // namespace warp_mapped

// ===========================================================================
// bucketing: thread / wavefront / chunk schedules by degree class
// ===========================================================================
namespace bucketing {

template <advance_direction_t direction,
          advance_io_type_t input_type,
          advance_io_type_t output_type,
          typename graph_t,
          typename operator_t,
          typename frontier_t>
void execute(graph_t& G,
             operator_t op,
             frontier_t& input,
             frontier_t& output,
             gcuda::standard_context_t& context) {
  namespace k = detail::k;
  using vertex_t = typename graph_t::vertex_type;
  using edge_t = typename graph_t::edge_type;
  constexpr advance_io_type_t vin = advance_io_type_t::vertices;
  detail::frame_t<vertex_t> f;
  if (!detail::open_frame<input_type, output_type>(f, detail::sizing_t::packed, G, input, output, context))
    return;
  const auto hubs = detail::plan_hubs<vertex_t, edge_t>(
      G, f.n_in, detail::work_bound_of<input_type>(G, input, f.total), context);
  vertex_t* bins = reinterpret_cast<vertex_t*>(context.workspace().scratch(2 * f.n_in * sizeof(vertex_t)));
  vertex_t* small_q = bins;
  vertex_t* medium_q = bins + f.n_in;
  const unsigned persistent = (unsigned)context.compute_units() * 8u;

  hip::clocked_t clock(context);
  k::bucket_kernel<input_type><<<hip::grid_for(f.n_in, k::ADV_BLOCK, persistent), k::ADV_BLOCK, 0,
                                 context.stream()>>>(
      G, input.data(), f.n_in, small_q, medium_q, hubs.chunks, hubs.chunk_capacity, hubs.hub_threshold,
      hubs.chunk_edges, f.counters);
  GRX_HIP_CHECK(hipGetLastError());
  unsigned long long* m = hip::fetch_counters(context);
  const std::size_t n_small = (std::size_t)m[k::C_BUCKET0];
  const std::size_t n_medium = (std::size_t)m[k::C_BUCKET0 + 1];
  const unsigned long long n_chunks = m[k::C_CHUNKS];

  if (n_small)
    k::thread_mapped_kernel<false, vin, output_type>
        <<<hip::grid_for(n_small, k::ADV_BLOCK, persistent), k::ADV_BLOCK, 0, context.stream()>>>(
            G, op, small_q, n_small, (const edge_t*)nullptr, f.out_ptr, f.capacity, f.counters);
  if (n_medium)
    k::wave_mapped_kernel<vin, output_type>
        <<<hip::grid_for(n_medium, k::ADV_WAVES, persistent), k::ADV_BLOCK, 0, context.stream()>>>(
            G, op, medium_q, n_medium, f.out_ptr, f.capacity, f.counters);
  if (n_chunks)
    k::chunk_kernel<output_type>
        <<<(unsigned)context.compute_units() * context.options().chunk_blocks_per_cu, k::ADV_BLOCK, 0,
           context.stream()>>>(G, op, hubs.chunks, hubs.chunk_capacity, f.out_ptr, f.capacity, f.counters,
                               (long long)n_chunks);
  detail::close_frame<output_type>(clock, output, f, context);
}

}  // namespace bucketing

// ===========================================================================
// pull (advance_direction_t::backward): candidates in, newly hit candidates out
// ===========================================================================
namespace pull {

/**
 * @brief Pull advance.  `input` holds candidate DESTINATION vertices; for each one its
 * in-edges are walked (CSR view of an undirected graph = its transpose) and
 * op(in_neighbour, candidate, edge, weight) is called until it returns true; such
 * candidates are written, packed, to `output`.  The op is called at most once per in-edge
 * and never again for a candidate after its first true.  With an attached transpose the edge
 * id handed to the op is the position in the TRANSPOSED arrays (transposed_t::edge_ids maps it
 * back to the CSR edge).  The reference declares this
 * direction but throws for it (advance_direction_t::backward / optimized,
 * framework/operators/configs.hxx:58-62, advance/merge_path.hxx:41-56).
 *
 * `rejected` (optional): receives, packed, the candidates with at least one in-edge for which
 * the op never returned true -- the candidate list of the next pull level, so that a caller
 * alternating pull levels needs no separate compaction pass.
 */
template <advance_io_type_t input_type,
          advance_io_type_t output_type,
          typename graph_t,
          typename operator_t,
          typename frontier_t>
void execute(graph_t& G,
             operator_t op,
             frontier_t& input,
             frontier_t& output,
             gcuda::standard_context_t& context,
             frontier_t* rejected = nullptr) {
  namespace k = detail::k;
  using vertex_t = typename graph_t::vertex_type;
  error::throw_if_exception(!G.can_pull(),
                            "pull advance needs in-edges: the graph is marked directed and has no "
                            "attached transpose (graph::build::transpose(G, ctx).attach_to(G), or "
                            "G.properties.directed = false for a symmetric CSR)");
  auto Gin = G.in_edges();  // the graph whose out-edges are G's in-edges
  error::throw_if_exception(input_type != advance_io_type_t::vertices,
                            "pull advance takes a vertex frontier of candidates");
  detail::frame_t<vertex_t> f;  // at most every candidate is emitted once
  if (!detail::open_frame<advance_io_type_t::vertices, output_type>(f, detail::sizing_t::candidates, G, input,
                                                                    output, context))
    return;
  const unsigned long long n_in = f.n_in;
  if (rejected) {
    error::throw_if_exception(rejected->data() == input.data() && rejected->data() != nullptr,
                              "pull advance: `rejected` must not alias the candidates");
    if (rejected->get_capacity() < n_in)
      rejected->reserve(n_in);
  }
  auto* long_queue = reinterpret_cast<k::resume_t<vertex_t>*>(
      context.workspace().queue(n_in * sizeof(k::resume_t<vertex_t>)));
  const unsigned persistent = (unsigned)context.compute_units() * 8u;
  hip::clocked_t clock(context);
  const unsigned probe_grid = hip::grid_for(n_in, k::ADV_BLOCK, persistent);
  const unsigned long_grid = (unsigned)context.compute_units() * 4u;
  // a separate in-edge view: the emitted vertices' OUT-degrees (the next push's work) come from
  // the forward offsets; an undirected CSR is its own transpose and needs no second lookup
  const auto* fwd = G.has_in_edges() ? G.get_row_offsets() : nullptr;
  if (rejected) {
    k::pull_probe_kernel<output_type, true><<<probe_grid, k::ADV_BLOCK, 0, context.stream()>>>(
        Gin, op, input.data(), f.n_in, f.out_ptr, f.capacity, rejected->data(), long_queue, n_in, f.counters,
        fwd);
    k::pull_long_kernel<output_type, true><<<long_grid, k::ADV_BLOCK, 0, context.stream()>>>(
        Gin, op, long_queue, n_in, f.out_ptr, f.capacity, rejected->data(), n_in, f.counters, fwd);
  } else {
    k::pull_probe_kernel<output_type, false><<<probe_grid, k::ADV_BLOCK, 0, context.stream()>>>(
        Gin, op, input.data(), f.n_in, f.out_ptr, f.capacity, (vertex_t*)nullptr, long_queue, n_in,
        f.counters, fwd);
    k::pull_long_kernel<output_type, false><<<long_grid, k::ADV_BLOCK, 0, context.stream()>>>(
        Gin, op, long_queue, n_in, f.out_ptr, f.capacity, (vertex_t*)nullptr, 0ull, f.counters, fwd);
  }
  detail::close_frame<output_type>(clock, output, f, context);
  if (rejected) {
    rejected->set_number_of_elements((std::size_t)context.workspace().mirror()[k::C_BUCKET0]);
    error::throw_if_exception(context.workspace().mirror()[k::C_OVERFLOW] != 0,
                              "pull advance: rejected list overflow");
  }
}

/**
 * @brief A wide level of a search, pulled over the id range [0, n) of a graph that is its OWN
 * transpose (the caller's knowledge: nothing is checked here) -- no candidate list, no output
 * frontier (advance_kernels.hxx: pull_range_kernel).  For every v < n that is not `labelled(v)`
 * the row of v is read from the front; at the first neighbour in the current frontier `label(v)` is
 * called and the row is left.  A neighbour u is in the frontier when its bit of `snapshot` is set
 * ("u was labelled when the level began"; u below the snapshot's limit) or, beyond the snapshot, when
 * `in_level(u)` says so -- the exact "u's label is this level's", which label() never changes.
 * `snapshot` must be EXACT for every id below its limit (settled.hxx: settled_snapshot_t, what
 * settled_filter_t::refresh() returns for this level) -- not the one-sided hint an advance takes: a
 * frontier vertex whose bit is missing is not seen by its neighbours.
 * One 1024-thread workgroup per CU keeps the snapshot in its LDS (at most settled_max_ids bits).
 * Only enqueues and leaves the kernel clock running: the operator that names what the level found
 * (filter::select_range) is its hand-off, as for an advance without an output.
 */
template <typename graph_t, typename vertex_t, typename labelled_t, typename in_level_t, typename label_t>
void enqueue_range(graph_t& G, std::size_t n, settled_snapshot_t<vertex_t> exact_snapshot, labelled_t labelled,
                   in_level_t in_level, label_t label, gcuda::standard_context_t& context) {
  namespace k = detail::k;
  if (n == 0)
    return;
  settled_view_t<vertex_t> snapshot = exact_snapshot.exact;
  if (!snapshot.bits)
    snapshot.limit = 0;
  error::throw_if_exception((std::size_t)snapshot.limit > settled_max_ids || snapshot.limit % 128 != 0,
                            "pull advance: the snapshot does not fit the LDS image");
  auto kernel = k::pull_range_kernel<graph_t, vertex_t, labelled_t, in_level_t, label_t>;
  const std::size_t lds = snapshot.limit > 0 ? (std::size_t)snapshot.limit / 8 : 16;
  static detail::lds_opt_in_t opt_in;  // of this instantiation of the kernel
  error::throw_if_exception(!opt_in.fits(reinterpret_cast<const void*>(kernel), lds, context),
                            "pull advance: the snapshot does not fit the LDS image");
  hip::clocked_t clock(context);
  kernel<<<hip::grid_for(n, k::SET_BLOCK, (unsigned)context.compute_units()), k::SET_BLOCK, lds,
           context.stream()>>>(G, n, snapshot, labelled, in_level, label);
  GRX_HIP_CHECK(hipGetLastError());
}

/// What sssp_pull_kernel walks: every row of the graph's own offsets as 8-byte {neighbour, weight}
/// entries sorted by ascending weight, and the first weight of every row.
struct light_rows_t {
  const unsigned long long* records = nullptr;
  const float* lightest = nullptr;
  explicit operator bool() const { return records != nullptr && lightest != nullptr; }
};

/**
 * @brief A wide SSSP round, pulled over the id range [0, n) of a graph that is its OWN transpose with
 * EQUAL weights in both directions (the caller's knowledge: nothing is checked here) -- no candidate
 * list, no output frontier, no atomics (advance_kernels.hxx: sssp_pull_kernel).  `packed`: the
 * client's 64-bit labels (order-preserving distance bits << 32 | round tag), `dmin_bits`: a device
 * word with the order-preserving bits of a lower bound of every frontier vertex's distance,
 * `far_bits`: the bits of "unreached", `this_round`: the tag a lowered label gets.
 * Only enqueues and leaves the kernel clock running: the operator that names what the round lowered
 * is its hand-off, which also carries counter C_EXAMINED to the host.
 */
template <typename graph_t>
void enqueue_sssp_range(graph_t& G, std::size_t n, light_rows_t rows, unsigned long long* packed,
                        const unsigned* dmin_bits, unsigned far_bits, unsigned this_round,
                        gcuda::standard_context_t& context) {
  namespace k = detail::k;
  using edge_t = typename graph_t::edge_type;
  if (n == 0)
    return;
  error::throw_if_exception(!rows || n > (std::size_t)G.get_number_of_vertices(),
                            "pull advance: no weight-sorted rows for this range");
  hip::clocked_t clock(context);
  k::sssp_pull_kernel<edge_t><<<hip::grid_for(n, k::SSSP_PULL_BLOCK, (unsigned)context.compute_units() * 8u),
                               k::SSSP_PULL_BLOCK, 0, context.stream()>>>(
      G.get_row_offsets(), rows.records, rows.lightest, n, packed, dmin_bits, far_bits, this_round,
      context.workspace().counters(), (int)k::C_EXAMINED);
  GRX_HIP_CHECK(hipGetLastError());
}

}  // namespace pull

// ===========================================================================
// dispatch
// ===========================================================================

/**
 * @brief Frontier-level entry (reference advance.hxx:91-129).
 */
template <load_balance_t lb,
          advance_direction_t direction,
          advance_io_type_t input_type,
          advance_io_type_t output_type,
          typename graph_t,
          typename operator_t,
          typename frontier_t,
          typename work_tiles_t>
void execute(graph_t& G,
             operator_t op,
             frontier_t* input,
             frontier_t* output,
             work_tiles_t& segments,
             gcuda::multi_context_t& context) {
  error::throw_if_exception(context.size() != 1, "`context.size() != 1` not supported");
  error::throw_if_exception(direction == advance_direction_t::optimized,
                            "advance: the push/pull choice is the client's (see the direction-"
                            "optimising BFS in essentials_amd/csrc/clients.hxx); ask for forward or backward");
  if constexpr (direction == advance_direction_t::backward) {
    pull::execute<input_type, output_type>(G, op, *input, *output, *context.get_context(0));
    return;
  }
  error::throw_if_exception(input_type == advance_io_type_t::edges ||
                                output_type == advance_io_type_t::edges ||
                                output_type == advance_io_type_t::graph,
                            "Advance type not supported.");
  auto& ctx = *context.get_context(0);
  constexpr load_balance_t schedule = GRX_LB_EFFECTIVE(lb);
  // every edge of the graph, nothing written: the order of the calls is the engine's choice, and
  // grouped by destination the functor's atomics combine (operators/by_destination.hxx)
  if constexpr (input_type == advance_io_type_t::graph && output_type == advance_io_type_t::none) {
    if (const void* items =
            by_destination::prepared(G, ctx.workspace().by_destination().current_run, ctx)) {
      hip::clocked_t clock(ctx);
      by_destination::enqueue(G, items, op, ctx);
      detail::close_frame<output_type>(clock, *output, detail::frame_t<typename graph_t::vertex_type>(), ctx,
                                       /*may_defer=*/true);
      return;
    }
  }
  // deterministic output positions exist only for merge_path / thread_mapped / block_mapped
  const bool holes = ctx.options().holes_layout && output_type != advance_io_type_t::none;

  if constexpr (schedule == load_balance_t::block_mapped) {
    block_mapped::execute<direction, input_type, output_type, false>(G, op, *input, *output, ctx);
  } else if constexpr (schedule == load_balance_t::work_stealing) {
    block_mapped::execute<direction, input_type, output_type, true>(G, op, *input, *output, ctx);
  } else if constexpr (schedule == load_balance_t::merge_path ||
                       schedule == load_balance_t::merge_path_v2) {
    merge_path::execute<direction, input_type, output_type>(G, op, *input, *output, segments, ctx);
  } else if constexpr (schedule == load_balance_t::thread_mapped) {
    thread_mapped::execute<direction, input_type, output_type>(G, op, *input, *output, segments, ctx);
  } else if constexpr (schedule == load_balance_t::warp_mapped) {
    if (holes)
      merge_path::execute<direction, input_type, output_type>(G, op, *input, *output, segments, ctx);
    else
      warp_mapped::execute<direction, input_type, output_type>(G, op, *input, *output, ctx);
  } else if constexpr (schedule == load_balance_t::bucketing) {
    if (holes)
      merge_path::execute<direction, input_type, output_type>(G, op, *input, *output, segments, ctx);
    else
      bucketing::execute<direction, input_type, output_type>(G, op, *input, *output, ctx);
  } else {
    error::throw_if_exception(true, "Advance type not supported.");
  }
}

/**
 * @brief Enactor-level entry (reference advance.hxx:192-221): uses the enactor's
 * input/output frontiers and scan workspace, then swaps the buffers.
 */
template <load_balance_t lb = load_balance_t::merge_path,
          advance_direction_t direction = advance_direction_t::forward,
          advance_io_type_t input_type = advance_io_type_t::vertices,
          advance_io_type_t output_type = advance_io_type_t::vertices,
          typename graph_t,
          typename enactor_type,
          typename operator_type>
void execute(graph_t& G,
             enactor_type* E,
             operator_type op,
             gcuda::multi_context_t& context,
             bool swap_buffers = true) {
  if constexpr (input_type == advance_io_type_t::graph && output_type == advance_io_type_t::none)
    context.get_context(0)->workspace().by_destination().current_run = E->unique_id;
  execute<lb, direction, input_type, output_type>(G, op, E->get_input_frontier(),
                                                  E->get_output_frontier(),
                                                  E->scanned_work_domain, context);
  if constexpr (input_type == advance_io_type_t::graph && output_type == advance_io_type_t::none)
    context.get_context(0)->workspace().by_destination().current_run = 0;
  if (swap_buffers && (output_type != advance_io_type_t::none))
    E->swap_frontier_buffers();
}

}  // namespace advance
}  // namespace operators
}  // namespace gunrock

/**
 * @file filter.hxx
 * @brief operators::filter::execute -- predicate-based frontier culling, and
 * operators::uniquify::execute -- duplicate removal.
 *
 * API of reference framework/operators/filter/filter.hxx:59-86,128-152 and
 * framework/operators/uniquify/uniquify.hxx:15-72.  Contracts kept: the predicate
 * is called exactly once per VALID element and never on invalid ones
 * (filter/predicated.hxx:24-26, bypass.hxx:29-34); bypass keeps the length and
 * may run in place; predicated / remove / compact are stable and shrink the
 * frontier; buffers are swapped afterwards unless swap_buffers == false.
 * The three culling variants share one hand-written two-pass ballot compaction
 * (gunrock/hip/kernels/compact_kernels.hxx).
 *
 * Reference defects NOT replicated (SURVEY.md 8a'): q2 -- `unique` leaves its
 * result in the frontier that is active after the call; q3 -- `unique_copy`
 * measures the new size on the output.
 */
#pragma once

#include <gunrock/framework/operators/advance.hxx>
#include <gunrock/framework/operators/configs.hxx>
#include <gunrock/hip/context.hxx>
#include <gunrock/hip/hand_off.hxx>
#include <gunrock/hip/kernels/advance_kernels.hxx>
#include <gunrock/hip/kernels/compact_kernels.hxx>

namespace gunrock {
namespace operators {

namespace detail {

/**
 * @brief out[0..m) = the elements in[i] with flag(i, in[i]) true, in order.
 * `in` and `out` must not alias.  Returns m.  One stream synchronise.
 */
template <typename type_t, typename flag_t>
std::size_t stable_select(const type_t* in, std::size_t n, type_t* out, flag_t flag,
                          gcuda::standard_context_t& ctx) {
  namespace k = ::gunrock::hip::kernels;
  if (n == 0)
    return 0;
  auto& ws = ctx.workspace();
  const std::size_t tiles = k::compaction_tiles(n);
  error::throw_if_exception(n >= (1ull << 32), "filter: more than 2^32 elements");
  // scratch layout: [words: tiles*16 u64][counts: tiles+1 u32][rocprim temp]
  const std::size_t words_bytes = tiles * k::CMP_WORDS * sizeof(unsigned long long);
  const std::size_t counts_bytes = ((tiles + 1) * sizeof(unsigned) + 15) & ~std::size_t(15);
  unsigned* probe = nullptr;
  const std::size_t scan_bytes = hip::exclusive_sum_temp_bytes(probe, probe, 0u, tiles + 1);
  unsigned char* base =
      reinterpret_cast<unsigned char*>(ws.scratch(words_bytes + counts_bytes + scan_bytes + 64));
  auto* words = reinterpret_cast<unsigned long long*>(base);
  auto* counts = reinterpret_cast<unsigned*>(base + words_bytes);
  void* temp = base + words_bytes + counts_bytes;

  GRX_HIP_CHECK(hipMemsetAsync(counts + tiles, 0, sizeof(unsigned), ctx.stream()));
  k::flag_kernel<<<(unsigned)tiles, k::CMP_BLOCK, 0, ctx.stream()>>>(in, n, words, counts, flag);
  GRX_HIP_CHECK(hipGetLastError());
  hip::exclusive_sum(temp, scan_bytes, counts, counts, 0u, tiles + 1, ctx.stream());
  unsigned* landing = reinterpret_cast<unsigned*>(ws.mirror() + 25);
  GRX_HIP_CHECK(hipMemcpyAsync(landing, counts + tiles, sizeof(unsigned), hipMemcpyDeviceToHost,
                               ctx.stream()));
  k::place_kernel<<<(unsigned)tiles, k::CMP_BLOCK, 0, ctx.stream()>>>(in, n, words, counts, out);
  GRX_HIP_CHECK(hipGetLastError());
  ctx.synchronize();
  return (std::size_t)*landing;
}

}  // namespace detail

namespace filter {

namespace bypass {
template <typename graph_t, typename operator_t, typename frontier_t>
void execute(graph_t&, operator_t op, frontier_t* input, frontier_t* output,
             gcuda::standard_context_t& context) {
  namespace k = ::gunrock::hip::kernels;
  const std::size_t n = input->get_number_of_elements();
  const unsigned long long hint = input->work_hint();
  if (output->get_capacity() < n)
    output->reserve(n);
  output->set_number_of_elements(n);
  output->set_work_hint(hint);  // elements are only removed: the bound still holds
  if (n) {
    std::size_t g = (n + k::CMP_BLOCK - 1) / k::CMP_BLOCK;
    const std::size_t cap = (std::size_t)context.compute_units() * 16;
    k::bypass_kernel<<<(unsigned)(g > cap ? cap : g), k::CMP_BLOCK, 0, context.stream()>>>(
        input->data(), n, output->data(), op);
    GRX_HIP_CHECK(hipGetLastError());
  }
  context.synchronize();
}
/// In-place form (reference filter/bypass.hxx:48-55).
template <typename graph_t, typename operator_t, typename frontier_t>
void execute(graph_t& G, operator_t op, frontier_t* input, gcuda::standard_context_t& context) {
  execute(G, op, input, input, context);
}
}  // namespace bypass

namespace compact {
template <typename graph_t, typename operator_t, typename frontier_t>
void execute(graph_t&, operator_t op, frontier_t* input, frontier_t* output,
             gcuda::standard_context_t& context) {
  using type_t = typename frontier_t::type_t;
  const std::size_t n = input->get_number_of_elements();
  error::throw_if_exception(input->data() == output->data() && n,
                            "filter: culling variants need distinct input and output frontiers");
  if (output->get_capacity() < n)
    output->reserve(n);
  auto keep = [op] __device__(std::size_t, type_t const& v) mutable -> bool {
    return util::limits::is_valid(v) ? op(v) : false;
  };
  const unsigned long long hint = input->work_hint();
  output->set_number_of_elements(
      operators::detail::stable_select(input->data(), n, output->data(), keep, context));
  output->set_work_hint(hint);
}
}  // namespace compact

namespace predicated {
template <typename graph_t, typename operator_t, typename frontier_t>
void execute(graph_t& G, operator_t op, frontier_t* input, frontier_t* output,
             gcuda::standard_context_t& context) {
  compact::execute(G, op, input, output, context);
}
}  // namespace predicated

namespace remove {
template <typename graph_t, typename operator_t, typename frontier_t>
void execute(graph_t& G, operator_t op, frontier_t* input, frontier_t* output,
             gcuda::standard_context_t& context) {
  compact::execute(G, op, input, output, context);
}
}  // namespace remove

/**
 * @brief output <- the vertices v in [0, n) with pred(v), and output's work hint <- the sum of their
 * degrees: what `output.sequence(0, n)` followed by filter::execute<predicated>(G, pred, ...) yields
 * as a SET (reference frontier.hxx sequence + filter/predicated.hxx:24-38), in one pass and with
 * ids ascending inside every run of 8192 (4096 with `narrow_claims`) candidates (compact_kernels.hxx: select_range_kernel).
 * The engine extension behind "run a wide level without an output frontier, then name what it found".
 * pred is called exactly once per v, in no particular order.  Synchronous.
 */
template <bool narrow_claims = false, typename graph_t, typename pred_t, typename frontier_t,
          typename each_t = ::gunrock::hip::kernels::select_no_each_t,
          typename bit_t = ::gunrock::hip::kernels::select_no_bit_t>
void select_range(graph_t& G, std::size_t n, pred_t pred, frontier_t& output,
                  gcuda::standard_context_t& context, each_t each = each_t(), bit_t bit = bit_t(),
                  unsigned long long* bit_words = nullptr, std::size_t bit_limit = 0,
                  std::size_t n_visit = 0) {
  namespace k = ::gunrock::hip::kernels;
  using vertex_t = typename frontier_t::type_t;
  // side products (compact_kernels.hxx): `each` for every id below n_visit (>= n; default n), bit i
  // of bit_words <- bit(i) for i < bit_limit (a multiple of 64, <= the ids visited)
  if (n_visit < n)
    n_visit = n;
  if (n_visit < bit_limit)
    n_visit = bit_limit;
  if (n_visit == 0) {
    output.set_number_of_elements(0);
    output.set_work_hint(0);
    return;
  }
  if (output.get_capacity() < n)  // at most every candidate is selected: the pass runs ONCE
    output.reserve(n);
  constexpr int items = narrow_claims ? k::SEL_ITEMS_NARROW : k::SEL_ITEMS_WIDE;
  const std::size_t chunks = (n_visit + (std::size_t)k::SEL_BLOCK * items - 1) / ((std::size_t)k::SEL_BLOCK * items);
  const std::size_t cap = (std::size_t)context.compute_units() * 2;
  hip::clocked_t clock(context);  // it IS a level's output path: timed with the advances
  k::select_range_kernel<vertex_t, items><<<(unsigned)(chunks < cap ? chunks : cap), k::SEL_BLOCK, 0,
                                     context.stream()>>>(G, n_visit, pred, output.data(), output.get_capacity(),
                                                         context.workspace().counters(), (int)k::C_OUT,
                                                         (int)k::C_NEXT_WORK, (int)k::C_OVERFLOW, n, each, bit,
                                                         bit_words, bit_limit);
  GRX_HIP_CHECK(hipGetLastError());
  clock.stop();
  unsigned long long* m = hip::fetch_counters(context);
  context.kernel_clock().collect();
  error::throw_if_exception(m[k::C_OVERFLOW] != 0, "select_range: output frontier capacity exceeded");
  output.set_number_of_elements((std::size_t)m[k::C_OUT]);
  output.set_work_hint(m[k::C_NEXT_WORK]);
  output.set_ascending(true);
}

/**
 * @brief The two passes in front of a near / far selection (compact_kernels.hxx, near_far.hxx):
 * `visit(v)` for every v in [0, n) returns the distance code of a pending v, -1 otherwise; then `*threshold` <- the smallest code at which the pending work reaches
 * the share `frac` of its total (NEAR_ALL when the total is below `min_total`), and the total to
 * counter C_PENDING.  `bins`: NEAR_BINS device words, zero on entry and on exit.  Only enqueues: the
 * select_range that follows on the same stream, with the predicate "pending and code <= *threshold",
 * is the hand-off.
 * `visit(v, bits)` also hands back the order-preserving bits of v's distance.  With `lowest` not null
 * (a client that may pull the next round) the same pass leaves *lowest <- min(*lowest, the bits of
 * every pending v) and the degree sum of the ids whose bits are `far_bits` in counter C_FAR_WORK, which
 * the same hand-off carries; `rearm` (the word the NEXT call reduces into) is set to 0xffffffff.
 */
template <typename graph_t, typename visit_t>
void choose_near(graph_t& G, std::size_t n, visit_t visit, unsigned long long* bins, unsigned* threshold, unsigned long long min_total, double frac,
                 gcuda::standard_context_t& context, unsigned* lowest = nullptr, unsigned far_bits = 0,
                 unsigned* rearm = nullptr) {
  namespace k = ::gunrock::hip::kernels;
  using vertex_t = typename graph_t::vertex_type;
  const unsigned grid = hip::grid_for(n, k::NEAR_BLOCK, (unsigned)context.compute_units() * 2);
  k::near_scan_kernel<vertex_t><<<grid, k::NEAR_BLOCK, 0, context.stream()>>>(
      G, n, visit, bins, lowest, far_bits, context.workspace().counters() + k::C_FAR_WORK);
  GRX_HIP_CHECK(hipGetLastError());
  k::near_choose_kernel<0><<<1, k::NEAR_BLOCK, 0, context.stream()>>>(
      bins, threshold, context.workspace().counters() + k::C_PENDING, min_total, frac, rearm);
  GRX_HIP_CHECK(hipGetLastError());
}

/// Frontier-level entry (reference filter.hxx:59-86).
template <filter_algorithm_t alg_type, typename graph_t, typename operator_t, typename frontier_t>
void execute(graph_t& G, operator_t op, frontier_t* input, frontier_t* output,
             gcuda::multi_context_t& context) {
  error::throw_if_exception(context.size() != 1, "`context.size() != 1` not supported");
  auto& ctx = *context.get_context(0);
  if constexpr (alg_type == filter_algorithm_t::compact)
    compact::execute(G, op, input, output, ctx);
  else if constexpr (alg_type == filter_algorithm_t::predicated)
    predicated::execute(G, op, input, output, ctx);
  else if constexpr (alg_type == filter_algorithm_t::bypass)
    bypass::execute(G, op, input, output, ctx);
  else if constexpr (alg_type == filter_algorithm_t::remove)
    remove::execute(G, op, input, output, ctx);
  else
    error::throw_if_exception(true, "Filter type not supported.");
}

/// Enactor-level entry (reference filter.hxx:128-152).
template <filter_algorithm_t alg_type, typename graph_t, typename enactor_type, typename operator_t>
void execute(graph_t& G, enactor_type* E, operator_t op, gcuda::multi_context_t& context,
             bool swap_buffers = true) {
  execute<alg_type>(G, op, E->get_input_frontier(), E->get_output_frontier(), context);
  if (swap_buffers)
    E->swap_frontier_buffers();
}

}  // namespace filter

namespace uniquify {

/**
 * @brief Frontier-level entry (reference uniquify.hxx:15-42).  Unless
 * best-effort, the input is radix-sorted first (rocPRIM) so that equal ids are
 * adjacent; then consecutive duplicates are dropped.
 *   unique      : the result replaces the contents of `input` (in place)
 *   unique_copy : the result is written to `output`
 */
template <uniquify_algorithm_t type, typename frontier_t>
void execute(frontier_t* input, frontier_t* output, gcuda::multi_context_t& context,
             bool best_effort_uniquification = false, const float uniquification_percent = 100) {
  using type_t = typename frontier_t::type_t;
  error::throw_if_exception(context.size() != 1, "`context.size() != 1` not supported");
  auto& ctx = *context.get_context(0);
  const std::size_t n = input->get_number_of_elements();
  if (output->get_capacity() < n)
    output->reserve(n);
  if (n == 0) {
    if (type == uniquify_algorithm_t::unique_copy)
      output->set_number_of_elements(0);
    return;
  }
  const type_t* src = input->data();
  if (!best_effort_uniquification && uniquification_percent == 100) {
    // sort input -> output storage, then select back into input storage (or the reverse)
    const std::size_t bytes = hip::radix_sort_temp_bytes<type_t>(n);
    void* temp = ctx.workspace().scratch(bytes);
    hip::radix_sort_keys(temp, bytes, input->data(), output->data(), n,
                         hip::sort_order_t::ascending, ctx.stream());
    if (type == uniquify_algorithm_t::unique) {
      src = output->data();  // sorted copy; result goes back into input
    } else {
      // result must land in output: move the sorted run back to input first
      GRX_HIP_CHECK(hipMemcpyAsync(input->data(), output->data(), n * sizeof(type_t),
                                   hipMemcpyDeviceToDevice, ctx.stream()));
      src = input->data();
    }
  } else if (type == uniquify_algorithm_t::unique) {
    // in place without a sort: stage a copy in output storage
    GRX_HIP_CHECK(hipMemcpyAsync(output->data(), input->data(), n * sizeof(type_t),
                                 hipMemcpyDeviceToDevice, ctx.stream()));
    src = output->data();
  }
  type_t* dst = (type == uniquify_algorithm_t::unique) ? input->data() : output->data();
  auto first_of_run = [src] __device__(std::size_t i, type_t const& v) -> bool {
    return i == 0 || src[i - 1] != v;
  };
  const unsigned long long hint = input->work_hint();
  const std::size_t m = operators::detail::stable_select(src, n, dst, first_of_run, ctx);
  if (type == uniquify_algorithm_t::unique) {
    input->set_number_of_elements(m);
    input->set_work_hint(hint);
  } else {
    output->set_number_of_elements(m);
    output->set_work_hint(hint);
  }
}

/**
 * @brief Enactor-level entry (reference uniquify.hxx:44-72).  `unique` works in
 * place on the active frontier, so no swap follows it; `unique_copy` fills the
 * inactive frontier and swaps (unless swap_buffers == false).
 */
template <uniquify_algorithm_t type = uniquify_algorithm_t::unique, typename enactor_type>
void execute(enactor_type* E, gcuda::multi_context_t& context,
             bool best_effort_uniquification = false, const float uniquification_percent = 100,
             bool swap_buffers = true) {
  if (!best_effort_uniquification)
    error::throw_if_exception(uniquification_percent < 0 || uniquification_percent > 100,
                              "Uniquification percentage must be a +ve float between 0 and 100.");
  execute<type>(E->get_input_frontier(), E->get_output_frontier(), context,
                best_effort_uniquification, uniquification_percent);
  if (swap_buffers && type == uniquify_algorithm_t::unique_copy)
    E->swap_frontier_buffers();
}

}  // namespace uniquify

namespace parallel_for {

namespace detail {
template <typename op_t>
__global__ void __launch_bounds__(256) for_kernel(std::size_t n, op_t op) {
  for (std::size_t i = blockIdx.x * (std::size_t)blockDim.x + threadIdx.x; i < n;
       i += (std::size_t)gridDim.x * blockDim.x)
    op(i);
}
template <typename type_t, typename op_t>
__global__ void __launch_bounds__(256) for_element_kernel(const type_t* f, std::size_t n, op_t op) {
  for (std::size_t i = blockIdx.x * (std::size_t)blockDim.x + threadIdx.x; i < n;
       i += (std::size_t)gridDim.x * blockDim.x) {
    type_t v = f[i];
    if (util::limits::is_valid(v))
      op(v);
  }
}
}  // namespace detail

/**
 * @brief for each vertex / edge / weight of a graph, or (type == element) for
 * each valid element of a frontier (reference for/for.hxx:28-96).  The functor
 * receives the id (vertex, edge), the weight value, or the frontier element.
 */
template <parallel_for_each_t type, typename graph_or_frontier_t, typename operator_t>
void execute(graph_or_frontier_t& X, operator_t op, gcuda::multi_context_t& context) {
  error::throw_if_exception(context.size() != 1, "`context.size() != 1` not supported");
  auto& ctx = *context.get_context(0);
  const std::size_t cap = (std::size_t)ctx.compute_units() * 16;
  if constexpr (type == parallel_for_each_t::element) {
    const std::size_t n = X.get_number_of_elements();
    if (n) {
      std::size_t g = (n + 255) / 256;
      detail::for_element_kernel<<<(unsigned)(g > cap ? cap : g), 256, 0, ctx.stream()>>>(
          X.data(), n, op);
      GRX_HIP_CHECK(hipGetLastError());
    }
  } else {
    using vertex_t = typename graph_or_frontier_t::vertex_type;
    using edge_t = typename graph_or_frontier_t::edge_type;
    const std::size_t n = (type == parallel_for_each_t::vertex)
                              ? (std::size_t)X.get_number_of_vertices()
                              : (std::size_t)X.get_number_of_edges();
    if (n) {
      std::size_t g = (n + 255) / 256;
      const unsigned grid = (unsigned)(g > cap ? cap : g);
      if constexpr (type == parallel_for_each_t::vertex) {
        auto body = [op] __device__(std::size_t i) mutable { vertex_t v = (vertex_t)i; op(v); };
        detail::for_kernel<<<grid, 256, 0, ctx.stream()>>>(n, body);
      } else if constexpr (type == parallel_for_each_t::edge) {
        auto body = [op] __device__(std::size_t i) mutable { edge_t e = (edge_t)i; op(e); };
        detail::for_kernel<<<grid, 256, 0, ctx.stream()>>>(n, body);
      } else {
        auto G = X;
        auto body = [op, G] __device__(std::size_t i) mutable {
          auto w = G.get_edge_weight((edge_t)i);
          op(w);
        };
        detail::for_kernel<<<grid, 256, 0, ctx.stream()>>>(n, body);
      }
      GRX_HIP_CHECK(hipGetLastError());
    }
  }
  ctx.synchronize();
}

}  // namespace parallel_for

}  // namespace operators
}  // namespace gunrock

/** @file capi_sample.hip  grx_neighbor_sample: multi-hop fan-out neighbour sampling without
 * replacement, every draw a function of (seed, vertex, hop, attempt), so a row's sample is the same
 * bits in every call, batch and schedule (hip/kernels/sample_kernels.hxx).  No reference counterpart.
 * Per hop: count + scan + the rows by lane-group class, hand-off 1 (the hop's edges, the rows per
 * class), the all-row copies and the pickers into the hop's own arrays, the claim of unseen
 * vertices, hand-off 2 (the new vertices, the failure flag), their sort and local ids, and the fill
 * of the caller's arrays.  Nothing of a hop reaches caller memory before both counts are known. */
#include "capi_batch.hxx"

#define GRX_WALK_DEFINITION_ONLY  // the draws of walk_kernels.hxx; its kernels live in capi_walk.hip
#include <gunrock/hip/kernels/sample_kernels.hxx>

#include <string>
#include <vector>

using namespace essentials_amd;

namespace k = gunrock::hip::kernels;

namespace {

/// F + 1 scan inputs: the entries of frontier row i for i < F, 0 at i == F.
struct row_counts_t {
  const int32_t* counts;
  int32_t F;
  __host__ __device__ int32_t operator()(int32_t i) const { return i < F ? counts[i] : 0; }
};

int runtime_error(const std::string& why) {
  last_error() = why;
  return GRX_ERR_RUNTIME;
}

/// Launch the picker of width G over one class: tables for the class's largest m, as many groups
/// per workgroup as the LDS holds.
template <int G>
void launch_pick(gcuda::standard_context_t& sc, const k::sample_args_t& a, const int32_t* order, int32_t begin,
                 int32_t count, int32_t largest_m, int max_lds) {
  const int32_t slots = k::sample_slots(largest_m, G);
  const std::size_t per_group = 2 * sizeof(int32_t) * (std::size_t)slots;
  const std::size_t fit = ((std::size_t)max_lds - 256) / per_group;  // the static part stays below 256 bytes
  error::throw_if_exception(fit < 1, "grx_neighbor_sample: a row's table does not fit the LDS");
  const int groups = (int)std::min<std::size_t>(k::SAMPLE_BLOCK / G, fit);
  const int threads = (groups * G + 63) / 64 * 64;  // whole wavefronts; lanes behind the last table idle
  const std::size_t lds = per_group * (std::size_t)groups;
  GRX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k::sample_pick_kernel<G>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  k::sample_pick_kernel<G><<<grid_for((std::size_t)count, (std::size_t)groups, sc), threads, lds, sc.stream()>>>(
      a, order, begin, count, slots, groups);
}

}  // namespace

extern "C" int grx_neighbor_sample(grx_context_t ctx, grx_graph_t g, const int32_t* h_seeds, int32_t n_seeds,
                                   const int32_t* h_fanouts, int32_t n_hops, uint64_t seed, int32_t* d_nodes,
                                   int64_t node_capacity, int32_t* d_src, int32_t* d_dst, int32_t* d_entry,
                                   int64_t edge_capacity, int64_t* h_node_offsets, int64_t* h_edge_offsets,
                                   const grx_options* opt, grx_stats* stats) {
  if (!ctx || !g || !h_fanouts)
    return invalid("grx_neighbor_sample: NULL argument");
  if (n_seeds < 0)
    return invalid("grx_neighbor_sample: n_seeds < 0");
  if (!h_seeds && n_seeds != 0)
    return invalid("grx_neighbor_sample: h_seeds is NULL (every vertex) but n_seeds != 0");
  for (int32_t i = 0; i < n_seeds; ++i)
    if (h_seeds[i] < 0 || h_seeds[i] >= g->n_rows)
      return invalid("grx_neighbor_sample: seed out of range");
  if (n_hops < 1 || n_hops > k::SAMPLE_MAX_HOPS)
    return invalid("grx_neighbor_sample: n_hops must be in [1, 64]");
  for (int32_t h = 0; h < n_hops; ++h)
    if (h_fanouts[h] != -1 && (h_fanouts[h] < 1 || h_fanouts[h] > k::SAMPLE_MAX_FANOUT))
      return invalid("grx_neighbor_sample: a fan-out must be -1 (every entry) or in [1, 1024]");
  if (g->n_rows != g->n_cols)
    return invalid("grx_neighbor_sample: the graph is not square (n_rows != n_cols)");
  if (node_capacity < 0 || edge_capacity < 0)
    return invalid("grx_neighbor_sample: negative capacity");
  if (!d_nodes && !d_src && !d_dst && !d_entry && !h_node_offsets && !h_edge_offsets)
    return invalid("grx_neighbor_sample: all six outputs are NULL");
  const grx_options o = effective_options(opt);
  if (o.max_iterations != 0)
    return invalid("grx_neighbor_sample: max_iterations must be 0 (the hops are an argument)");
  const bool timed = o.collect_kernel_time != 0;
  return guarded([&] {
    if (stats)
      std::memset(stats, 0, sizeof *stats);
    if (h_node_offsets)
      std::fill(h_node_offsets, h_node_offsets + n_hops + 2, int64_t(0));
    if (h_edge_offsets)
      std::fill(h_edge_offsets, h_edge_offsets + n_hops + 1, int64_t(0));
    const int32_t n = g->n_rows;
    if (n == 0 || (h_seeds && n_seeds == 0))  // nobody to expand: nothing is written, nothing is launched
      return (int)GRX_OK;

    // level 0: the distinct seeds in list order
    std::vector<int32_t> seeds;
    if (h_seeds) {
      std::vector<bool> seen((std::size_t)n, false);
      for (int32_t i = 0; i < n_seeds; ++i)
        if (!seen[(std::size_t)h_seeds[i]]) {
          seen[(std::size_t)h_seeds[i]] = true;
          seeds.push_back(h_seeds[i]);
        }
    }
    const int32_t n0 = h_seeds ? (int32_t)seeds.size() : n;
    if (d_nodes && (int64_t)n0 > node_capacity)
      return runtime_error("grx_neighbor_sample: level 0 needs node_capacity " + std::to_string(n0));
    const bool want_edges = d_src || d_dst || d_entry;

    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();
    int max_lds = 0;
    {
      int dev = 0;
      GRX_HIP_CHECK(hipGetDevice(&dev));
      GRX_HIP_CHECK(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    }
    // test hook: the lane-group width of every row (0: by the rule)
    k::sample_rule_t rule = k::SAMPLE_RULE;
    switch (env_or("GRX_SAMPLE_GROUP", 0, 0, 256)) {
      case 0: break;
      case 8: rule = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX}; break;
      case 64: rule = {-1, INT32_MAX, -1, INT32_MAX}; break;
      case 256: rule = {-1, -1, -1, -1}; break;
      default: return invalid("grx_neighbor_sample: GRX_SAMPLE_GROUP must be 0, 8, 64 or 256");
    }

    call_clock_t clock(s, timed);
    clock.start();
    bool batch_open = false;  // a batch of launches ends at a hand-off and begins behind it
    auto open_batch = [&] {
      if (!batch_open)
        clock.begin_batch();
      batch_open = true;
    };
    auto close_batch = [&] {
      if (batch_open)
        clock.end_batch();
      batch_open = false;
    };
    int32_t launches = 0, expanding_hops = 0;
    int64_t nodes = n0, edges = 0;
    std::vector<int64_t> expanded((std::size_t)n_hops, 0);
    k::sample_counters_t h_ctr;
    std::memset(&h_ctr, 0, sizeof h_ctr);
    unsigned long long attempts = 0;
    std::string failure;
    {
      hip::device_array_t<int32_t> local((std::size_t)n);
      hip::device_array_t<int32_t> level((std::size_t)n0);  // the frontier: level h - 1
      hip::device_array_t<k::sample_counters_t> counters(1);
      hip::device_array_t<int32_t> d_seeds(seeds.size());
      k::sample_counters_t* ctr = counters.data();
      GRX_HIP_CHECK(hipMemsetAsync(local.data(), 0xff, sizeof(int32_t) * (std::size_t)n, s));
      GRX_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof *ctr, s));
      if (h_seeds)
        GRX_HIP_CHECK(hipMemcpyAsync(d_seeds.data(), seeds.data(), seeds.size() * sizeof(int32_t),
                                     hipMemcpyHostToDevice, s));
      open_batch();
      k::sample_seed_kernel<<<grid_for((std::size_t)n0, k::SAMPLE_BLOCK, sc), k::SAMPLE_BLOCK, 0, s>>>(
          h_seeds ? d_seeds.data() : nullptr, n0, level.data(), local.data(), d_nodes);
      GRX_HIP_CHECK(hipGetLastError());
      ++launches;
      if (h_node_offsets)
        h_node_offsets[1] = n0;

      int32_t F = n0;  // vertices of level h - 1
      for (int32_t h = 1; h <= n_hops; ++h) {
        const int32_t fan = h_fanouts[h - 1];
        expanded[(std::size_t)h - 1] = F;
        int32_t E = 0, C = 0;
        if (F > 0) {
          ++expanding_hops;
          // (a) entries per row, rows by class
          hip::device_array_t<int32_t> counts((std::size_t)F), row_off((std::size_t)F + 1), order((std::size_t)F);
          hip::device_array_t<unsigned char> cls((std::size_t)F), cls_sorted((std::size_t)F);
          GRX_HIP_CHECK(hipMemsetAsync(&ctr->claimed, 0, sizeof(unsigned) * (2 + k::SC_CLASSES), s));  // claimed, failed, rows
          k::sample_count_kernel<<<grid_for((std::size_t)F, k::SAMPLE_BLOCK, sc), k::SAMPLE_BLOCK, 0, s>>>(
              g->d_ap, level.data(), F, fan, rule, counts.data(), cls.data(), ctr);
          GRX_HIP_CHECK(hipGetLastError());
          ++launches;
          {
            auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int32_t>(0),
                                                       row_counts_t{counts.data(), F});
            std::size_t scan_bytes = hip::exclusive_sum_temp_bytes(in, row_off.data(), int32_t(0), (std::size_t)F + 1);
            std::size_t sort_bytes = 0;
            GRX_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, cls.data(), cls_sorted.data(),
                                                    rocprim::make_counting_iterator<int32_t>(0), order.data(),
                                                    (std::size_t)F, 0, k::SAMPLE_CLASS_BITS, s));
            hip::device_array_t<unsigned char> temp(std::max<std::size_t>(std::max(scan_bytes, sort_bytes), 256));
            hip::exclusive_sum(temp.data(), scan_bytes, in, row_off.data(), int32_t(0), (std::size_t)F + 1, s);
            GRX_HIP_CHECK(rocprim::radix_sort_pairs(temp.data(), sort_bytes, cls.data(), cls_sorted.data(),
                                                    rocprim::make_counting_iterator<int32_t>(0), order.data(),
                                                    (std::size_t)F, 0, k::SAMPLE_CLASS_BITS, s));
            // hand-off 1: the hop's edges and its rows per class
            close_batch();
            GRX_HIP_CHECK(hipMemcpyAsync(&E, row_off.data() + F, sizeof E, hipMemcpyDeviceToHost, s));
            GRX_HIP_CHECK(hipMemcpyAsync(&h_ctr, ctr, sizeof h_ctr, hipMemcpyDeviceToHost, s));
            GRX_HIP_CHECK(hipStreamSynchronize(s));
          }
          if (want_edges && edges + (int64_t)E > edge_capacity) {
            failure = "grx_neighbor_sample: hop " + std::to_string(h) + " needs edge_capacity " +
                      std::to_string(edges + (int64_t)E);
            break;
          }
          if (E > 0) {
            // (b) the hop's edges into arrays of its own, (c) the claim
            const int32_t room = (int32_t)std::min<int64_t>(E, (int64_t)n - nodes);
            hip::device_array_t<int32_t> t_src((std::size_t)E), t_entry((std::size_t)E), t_nbr((std::size_t)E);
            hip::device_array_t<int32_t> claimed((std::size_t)room), next((std::size_t)room);
            hip::device_array_t<unsigned char> sort_temp;
            const k::sample_args_t a{g->d_ap,      g->d_aj,        level.data(), row_off.data(), (int32_t)(nodes - F),
                                     fan,          (unsigned)h,    seed,         t_src.data(),   t_entry.data(),
                                     t_nbr.data(), ctr};
            open_batch();
            // the largest m a row of a class can have: the class's threshold, and never above the fan-out
            const int32_t most = std::max<int32_t>(fan, 1);
            int32_t begin = 0;
            for (int c = 0; c < k::SC_NONE; ++c) {
              const int32_t rows = (int32_t)h_ctr.rows[c];
              if (rows == 0)
                continue;
              switch (c) {
                case k::SC_COPY8:
                  k::sample_copy_kernel<8><<<grid_for((std::size_t)rows, k::SAMPLE_BLOCK / 8, sc), k::SAMPLE_BLOCK, 0, s>>>(
                      a, order.data(), begin, rows);
                  break;
                case k::SC_COPY64:
                  k::sample_copy_kernel<64><<<grid_for((std::size_t)rows, k::SAMPLE_BLOCK / 64, sc), k::SAMPLE_BLOCK, 0, s>>>(
                      a, order.data(), begin, rows);
                  break;
                case k::SC_COPY256:
                  k::sample_copy_kernel<256><<<grid_for((std::size_t)rows, 1, sc), k::SAMPLE_BLOCK, 0, s>>>(
                      a, order.data(), begin, rows);
                  break;
                case k::SC_PICK8:
                  launch_pick<8>(sc, a, order.data(), begin, rows, std::min(most, std::max(rule.pick8, 1)), max_lds);
                  break;
                case k::SC_PICK64:
                  launch_pick<64>(sc, a, order.data(), begin, rows, std::min(most, std::max(rule.pick64, 1)), max_lds);
                  break;
                default:
                  launch_pick<256>(sc, a, order.data(), begin, rows, most, max_lds);
                  break;
              }
              GRX_HIP_CHECK(hipGetLastError());
              ++launches;
              begin += rows;
            }
            if (room > 0) {
              k::sample_claim_kernel<<<grid_for((std::size_t)E, k::SAMPLE_BLOCK, sc), k::SAMPLE_BLOCK, 0, s>>>(
                  t_nbr.data(), E, local.data(), claimed.data(), room, ctr);
              GRX_HIP_CHECK(hipGetLastError());
              ++launches;
            }
            // hand-off 2: the new vertices, the attempts so far, the failure flag
            close_batch();
            GRX_HIP_CHECK(hipMemcpyAsync(&h_ctr, ctr, sizeof h_ctr, hipMemcpyDeviceToHost, s));
            GRX_HIP_CHECK(hipStreamSynchronize(s));
            attempts = h_ctr.attempts;
            C = (int32_t)h_ctr.claimed;
            if (h_ctr.failed) {
              failure = "grx_neighbor_sample: hop " + std::to_string(h) + ": a row met its attempt bound";
              break;
            }
            error::throw_if_exception(C > room, "grx_neighbor_sample: more new vertices than the graph has left");
            if (d_nodes && nodes + (int64_t)C > node_capacity) {
              failure = "grx_neighbor_sample: hop " + std::to_string(h) + " needs node_capacity " +
                        std::to_string(nodes + (int64_t)C);
              break;
            }
            open_batch();
            if (C > 0) {
              std::size_t bytes = 0;
              GRX_HIP_CHECK(rocprim::radix_sort_keys(nullptr, bytes, claimed.data(), next.data(), (std::size_t)C, 0, 32, s));
              sort_temp.resize(std::max<std::size_t>(bytes, 256));
              GRX_HIP_CHECK(rocprim::radix_sort_keys(sort_temp.data(), bytes, claimed.data(), next.data(), (std::size_t)C, 0, 32, s));
              k::sample_assign_kernel<<<grid_for((std::size_t)C, k::SAMPLE_BLOCK, sc), k::SAMPLE_BLOCK, 0, s>>>(
                  next.data(), C, (int32_t)nodes, local.data(), d_nodes);
              GRX_HIP_CHECK(hipGetLastError());
              ++launches;
            }
            // (d) the caller's arrays
            if (want_edges) {
              k::sample_fill_kernel<<<grid_for((std::size_t)E, k::SAMPLE_BLOCK, sc), k::SAMPLE_BLOCK, 0, s>>>(
                  t_src.data(), t_entry.data(), t_nbr.data(), E, local.data(), d_src ? d_src + edges : nullptr,
                  d_dst ? d_dst + edges : nullptr, d_entry ? d_entry + edges : nullptr);
              GRX_HIP_CHECK(hipGetLastError());
              ++launches;
            }
            GRX_HIP_CHECK(hipStreamSynchronize(s));  // the hop's arrays and the sort's storage go
            level = std::move(next);
          } else {
            attempts = h_ctr.attempts;
            open_batch();
          }
        }
        edges += E;
        nodes += C;
        F = C;
        if (h_edge_offsets)
          h_edge_offsets[h] = edges;
        if (h_node_offsets)
          h_node_offsets[h + 1] = nodes;
      }
      close_batch();
      GRX_HIP_CHECK(hipStreamSynchronize(s));
      clock.stop_and_wait();
    }
    hip::block_cache_t::instance().trim();
    if (!failure.empty())
      return runtime_error(failure);

    if (stats) {
      stats->elapsed_ms = clock.elapsed_ms();
      stats->advance_kernel_ms = clock.kernel_ms();
      stats->advance_launches = launches;
      stats->iterations = expanding_hops;
      stats->vertices_reached = nodes;
      stats->edges_traversed = edges;
      stats->edges_expanded = (int64_t)attempts;
      stats->levels_recorded = n_hops;
      for (int32_t h = 0; h < n_hops; ++h)
        stats->frontier_slots[h] = expanded[(std::size_t)h];
    }
    return (int)GRX_OK;
  });
}

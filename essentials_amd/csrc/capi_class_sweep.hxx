/**
 * @file capi_class_sweep.hxx
 * @brief Host side of the colour-class sweep that grx_lpa and grx_louvain share
 * (hip/kernels/class_sweep.hxx): the test hooks, the schedule -- grx_color, the sort of the
 * vertices by (colour, row-length bin), the launch plan of a sweep and what its overflow paths
 * need --, the launches of one sweep for a decision D, the score passes and Q.  Not installed.
 */
#pragma once

#include "capi_batch.hxx"

#include <gunrock/hip/kernels/class_sweep.hxx>

#include <string>
#include <vector>

namespace essentials_amd {

/// Test hooks and what the device allows.
struct sweep_limits_t {
  int32_t big_row;                 // <prefix>_BIG_ROW: longer rows get 1024 threads and the largest table
  unsigned long long narrow_edges; // <prefix>_NARROW_EDGES: the entries a class may have to run in the
                                   // one-workgroup kernel (0 sends every class to the wide kernels)
  int32_t slots;                   // <prefix>_LDS_SLOTS: the slots of the largest LDS table
};

inline sweep_limits_t sweep_limits(const char* prefix) {
  namespace k = gunrock::hip::kernels;
  const std::string p(prefix);
  sweep_limits_t lim;
  lim.big_row = (int32_t)env_or((p + "_BIG_ROW").c_str(), k::LPA_BIG_ROW, 1, INT32_MAX);
  lim.narrow_edges = (unsigned long long)env_or((p + "_NARROW_EDGES").c_str(), k::LPA_NARROW_EDGES, 0, 1ll << 30);
  int dev = 0, max_lds = 0;
  GRX_HIP_CHECK(hipGetDevice(&dev));
  GRX_HIP_CHECK(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  const long long most = ((long long)max_lds - 1024) / 8;  // a key and a sum; the static part stays below 1 KB
  lim.slots = (int32_t)env_or((p + "_LDS_SLOTS").c_str(), most, k::LPA_MIN_SLOTS, most);
  return lim;
}

/// Consecutive colour classes that one launch sequence serves: one wide class, or a run of small ones.
struct step_t {
  int32_t c0, c1;
  bool narrow;
};

/// The vertices of a graph by (colour class, bin) and the launch plan of a sweep over them.
struct class_schedule_t {
  int32_t n = 0, slots = 0, medium_slots = 0;
  std::size_t medium_lds = 0, big_lds = 0, narrow_lds = 0;
  bool lds_allowed = false;  // enqueue_sweep has set the kernels' dynamic LDS limits; one decision per schedule
  hip::device_array_t<unsigned> keys;  // sorted; free for the caller once the schedule is built
  hip::device_array_t<int32_t> order, starts;
  std::vector<int32_t> h_starts;
  std::vector<step_t> steps;
  hip::device_array_t<int32_t> pool;
  hip::device_array_t<unsigned long long> over;

  /// Colours `pattern` (rows ap[0 .. n]) and plans; `call` names the caller in messages.  Returns
  /// grx_color's code.  A class whose vertices have no entries decides nothing and is not planned.
  int build(grx_context_s* ctx, grx_graph_s* pattern, const int32_t* ap, int32_t n_, const sweep_limits_t& lim,
            call_clock_t& clock, int32_t& launches, const char* call) {
    namespace k = gunrock::hip::kernels;
    auto& sc = ctx->single();
    const hipStream_t s = sc.stream();
    n = n_;
    slots = lim.slots;
    lds_allowed = false;
    k::lpa_key_t key{nullptr, ap, {0, 0, 0}};
    key.b[0] = std::min(k::LPA_SMALL_ROW, lim.big_row);
    key.b[1] = std::min(k::LPA_WAVE_ROW, lim.big_row);
    key.b[2] = std::max(key.b[1], std::min(lim.big_row, lim.slots / 2));  // a medium row's table never overflows
    medium_slots = (int32_t)k::lpa_slots_for(key.b[2], lim.slots);
    medium_lds = 2 * sizeof(int32_t) * (std::size_t)medium_slots;
    big_lds = 2 * sizeof(int32_t) * (std::size_t)lim.slots;
    narrow_lds =
        std::max(big_lds, 2 * sizeof(int32_t) * (std::size_t)k::LPA_WAVE_SLOTS * (k::LPA_BIG_BLOCK / hip::wave_size));

    // 1. the colour classes
    hip::device_array_t<int32_t> color((std::size_t)n);
    int32_t num_colors = 0;
    if (int rc = grx_color(ctx, pattern, color.data(), &num_colors, nullptr, nullptr))
      return rc;
    key.color = color.data();
    const int32_t n_keys = num_colors * k::LPA_BINS;
    int bits = 1;
    while ((1ll << bits) < n_keys)
      ++bits;

    // 2. the vertices by (class, bin), ascending ids within; sizes and entry totals to the host
    keys = hip::device_array_t<unsigned>((std::size_t)n);
    order = hip::device_array_t<int32_t>((std::size_t)n);
    starts = hip::device_array_t<int32_t>((std::size_t)n_keys + 1);
    hip::device_array_t<unsigned long long> entries((std::size_t)n_keys);
    h_starts.resize((std::size_t)n_keys + 1);
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
          keys.data(), order.data(), ap, n, entries.data());
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
    steps.clear();
    unsigned long long pool_entries = 0;
    std::size_t over_rows = 0;
    for (int32_t c = 0; c < num_colors; ++c) {
      const int32_t* at = h_starts.data() + k::LPA_BINS * c;
      const unsigned long long* e = h_entries.data() + k::LPA_BINS * c;
      const int32_t size = at[k::LPA_BINS] - at[0];
      const unsigned long long class_entries = e[0] + e[1] + e[2] + e[3];
      if (size == 0 || class_entries == 0)  // nobody, or only vertices without entries
        continue;
      const bool narrow = lim.narrow_edges && size <= k::LPA_NARROW_VERTICES && class_entries <= lim.narrow_edges;
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
    error::throw_if_exception(pool_entries > (unsigned long long)INT32_MAX,
                              (std::string(call) + ": more entries than a CSR holds").c_str());
    pool = hip::device_array_t<int32_t>(4 * (std::size_t)pool_entries + 4);
    over = hip::device_array_t<unsigned long long>(over_rows + 1);
    return (int)GRX_OK;
  }
};

/// Enqueue one sweep of the schedule, which serves one decision D: per planned step either the one-workgroup kernel over its run of small
/// classes, or one launch per non-empty bin of its wide class (and the fallback kernel where the
/// class has big rows), followed by D's apply launch where it has one.
template <class D>
void enqueue_sweep(gcuda::standard_context_t& sc, class_schedule_t& sched, const typename D::state_t& st,
                   typename D::counters_t* ctr, int32_t& launches) {
  namespace k = gunrock::hip::kernels;
  const hipStream_t s = sc.stream();
  if (!sched.lds_allowed) {  // once per schedule: D's workgroup kernels may have the dynamic LDS it asks for
    GRX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k::sweep_block_kernel<D, k::LPA_BLOCK>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)sched.medium_lds));
    GRX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k::sweep_block_kernel<D, k::LPA_BIG_BLOCK>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)sched.big_lds));
    GRX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k::sweep_narrow_kernel<D>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)sched.narrow_lds));
    sched.lds_allowed = true;
  }
  const int32_t* rows = sched.order.data();
  for (const step_t& step : sched.steps) {
    if (step.narrow) {
      k::sweep_narrow_kernel<D><<<1, k::LPA_BIG_BLOCK, sched.narrow_lds, s>>>(
          st, rows, sched.starts.data(), step.c0, step.c1, sched.slots, sched.pool.data(), ctr);
      ++launches;
      continue;
    }
    const int32_t* at = sched.h_starts.data() + k::LPA_BINS * step.c0;
    if (const int32_t r = at[1] - at[0]) {
      k::sweep_group_kernel<D, k::LPA_SMALL>
          <<<grid_for((std::size_t)r, k::LPA_BLOCK / k::LPA_SMALL, sc), k::LPA_BLOCK, 0, s>>>(st, rows + at[0], r, ctr);
      ++launches;
    }
    if (const int32_t r = at[2] - at[1]) {
      k::sweep_group_kernel<D, hip::wave_size>
          <<<grid_for((std::size_t)r, k::LPA_BLOCK / hip::wave_size, sc), k::LPA_BLOCK, 0, s>>>(st, rows + at[1], r, ctr);
      ++launches;
    }
    if (const int32_t r = at[3] - at[2]) {
      k::sweep_block_kernel<D, k::LPA_BLOCK><<<grid_for((std::size_t)r, 1, sc), k::LPA_BLOCK, sched.medium_lds, s>>>(
          st, rows + at[2], r, sched.medium_slots, sched.over.data(), ctr);
      ++launches;
    }
    if (const int32_t r = at[4] - at[3]) {
      // the class's overflow list and its share of the pool start empty
      GRX_HIP_CHECK(hipMemsetAsync(&ctr->overflow_n, 0, 2 * sizeof(int), s));
      k::sweep_block_kernel<D, k::LPA_BIG_BLOCK><<<grid_for((std::size_t)r, 1, sc), k::LPA_BIG_BLOCK, sched.big_lds, s>>>(
          st, rows + at[3], r, sched.slots, sched.over.data(), ctr);
      k::sweep_fallback_kernel<D>
          <<<std::min<unsigned>((unsigned)r, (unsigned)sc.compute_units()), k::LPA_BIG_BLOCK, 0, s>>>(
              st, sched.over.data(), sched.pool.data(), ctr);
      launches += 2;
    }
    if constexpr (D::apply_kernel != nullptr) {  // the class is decided: its moves take effect
      const int32_t r = at[4] - at[0];
      D::apply_kernel<<<grid_for((std::size_t)r, k::LPA_BLOCK, sc), k::LPA_BLOCK, 0, s>>>(st, rows + at[0], r, ctr);
      ++launches;
    }
  }
}

/// Items of the big list of the score passes: a row above the segment length has at most
/// d / segment + 1 segments.
inline std::size_t big_list_size(int64_t entries) {
  return 2 * ((std::size_t)entries / gunrock::hip::kernels::LPA_INSIDE_SEGMENT) + 1;
}

/// Enqueue the score passes of `label` over the CSR (aw is not read unless WEIGHTED): I and S land
/// in ctr->inside and ctr->squares.  `big`: big_list_size(entries) items, ctr->big_n zero.  Returns
/// the launches.
template <bool WEIGHTED, class tot_t, class counters_t>
int32_t enqueue_score(gcuda::standard_context_t& sc, const int32_t* ap, const int32_t* aj, const int32_t* aw,
                      const int32_t* label, int32_t n, const tot_t* tot, int2* big, counters_t* ctr) {
  namespace k = gunrock::hip::kernels;
  const hipStream_t s = sc.stream();
  const unsigned grid = grid_for((std::size_t)n, k::LPA_BLOCK, sc);
  k::sweep_inside_kernel<WEIGHTED><<<grid, k::LPA_BLOCK, 0, s>>>(ap, aj, aw, label, n, big, ctr);
  k::sweep_inside_big_kernel<WEIGHTED>
      <<<(unsigned)sc.compute_units() * 4, k::LPA_BLOCK, 0, s>>>(ap, aj, aw, label, (const int2*)big, ctr);
  k::sweep_squares_kernel<<<grid, k::LPA_BLOCK, 0, s>>>(tot, n, ctr);
  return 3;
}

/// Q from its integer parts, in exactly this form.
inline double modularity_of(unsigned long long inside, unsigned long long squares, int64_t entries) {
  if (entries == 0)
    return 0.0;
  return (double)inside / (double)entries - (double)squares / ((double)entries * (double)entries);
}

}  // namespace essentials_amd

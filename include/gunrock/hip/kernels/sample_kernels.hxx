/**
 * @file sample_kernels.hxx
 * @brief Neighbour sampling (grx_neighbor_sample, include/essentials_amd.h): multi-hop fan-out
 * sampling without replacement, every draw a function of (seed, vertex, hop, attempt) alone.
 *
 * The first part of the file is the DEFINITION of a row's sample and compiles as plain C++
 * (tests/cpp/sample_pick_tests.cpp): the plan of a row (all / include / exclude and the number m of
 * distinct positions to find), the attempt bound, and the candidate of an attempt, which is
 * walk_kernels.hxx's draw keyed by the vertex.  The kernels below call exactly these.  A translation
 * unit that is not the home of the walk kernels defines GRX_WALK_DEFINITION_ONLY before including this.
 *
 * Kernels of a hop: the count pass (entries per frontier row, its lane-group class, the class
 * histogram), the all-row copy and the picker per lane-group width, the claim of unseen vertices,
 * the local ids of the sorted claims, and the fill that writes the caller's arrays.  The host scans
 * the counts and sorts the rows by class in between (rocPRIM) and reads two small records per hop.
 */
#pragma once

#include <cstdint>

#include <gunrock/hip/kernels/walk_kernels.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int SAMPLE_MAX_FANOUT = 1024;  // the largest k: part of the definition
constexpr int SAMPLE_MAX_HOPS = 64;      // grx_stats::frontier_slots

enum sample_mode_t : int { SAMPLE_ALL = 0, SAMPLE_INCLUDE = 1, SAMPLE_EXCLUDE = 2 };

struct sample_plan_t {
  int mode;
  long long m;  // distinct positions to find: <= d / 2; 0 for SAMPLE_ALL
};

/// What a row of `d` entries does under fan-out `k` (-1: every entry).
GRX_WALK_HD inline sample_plan_t sample_plan(long long d, long long k) {
  if (k < 0 || d <= k)
    return {SAMPLE_ALL, 0};
  if (2 * k <= d)
    return {SAMPLE_INCLUDE, k};
  return {SAMPLE_EXCLUDE, d - k};
}

/// Attempts a row may make before the call fails.
GRX_WALK_HD inline long long sample_attempt_bound(long long m) { return 64 * m + 1024; }

/// x_a of row v in hop h: r(v, h, a) scaled to [0, d).  The picker computes walk_stream(seed, v) once
/// per row and calls walk_draw and walk_pick_uniform per attempt: the same three functions.
GRX_WALK_HD inline long long sample_candidate(unsigned long long seed, unsigned long long v, unsigned hop,
                                              unsigned long long a, long long d) {
  return walk_pick_uniform(walk_draw(walk_stream(seed, v), hop, a), d);
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

#if defined(__HIPCC__)

#include <gunrock/hip/primitives.hxx>

namespace gunrock {
namespace hip {
namespace kernels {

constexpr int SAMPLE_BLOCK = 256;
constexpr int32_t SAMPLE_EMPTY = INT32_MAX;  // a free table slot: no position is this large
constexpr int SAMPLE_MIN_SLOTS = 16;

/// The lane-group class of a frontier row.
enum sample_class_t : int {
  SC_COPY8 = 0,
  SC_COPY64,
  SC_COPY256,
  SC_PICK8,
  SC_PICK64,
  SC_PICK256,
  SC_NONE,  // an empty row
  SC_CLASSES
};
constexpr int SAMPLE_CLASS_BITS = 3;

/// Which width a row goes to: an all-row by its length, an include row by its m, an exclude row by
/// d / 2 (it reads the whole row out).  A forced width (GRX_SAMPLE_GROUP) is the same rule with
/// thresholds of -1 and INT32_MAX.
struct sample_rule_t {
  int32_t copy8, copy64;  // d <= copy8: 8 lanes; d <= copy64: a wavefront; else a workgroup
  int32_t pick8, pick64;  // the same by m, or by d / 2
};
constexpr sample_rule_t SAMPLE_RULE = {16, 1024, 32, 256};

/// Device record of a call; the host reads it twice per hop.
struct sample_counters_t {
  unsigned long long attempts;   // sum of A over the picking rows, of d over the all-rows
  unsigned int claimed;          // vertices first named in this hop
  unsigned int failed;           // a row met its attempt bound, or a table filled up
  unsigned int rows[SC_CLASSES];  // this hop's frontier rows by class
};

struct sample_args_t {
  const int32_t* ap;
  const int32_t* aj;
  const int32_t* frontier;  // the vertices of level h - 1, in node-list order
  const int32_t* row_off;   // [F + 1]: where a frontier row's entries go in the hop's arrays
  int32_t first_local;      // local id of frontier[0]
  int32_t k;                // the hop's fan-out, -1: all
  unsigned hop;             // 1-based
  unsigned long long seed;
  int32_t* t_src;           // the hop's edges, E_h each
  int32_t* t_entry;
  int32_t* t_nbr;           // neighbours in the caller's numbering
  sample_counters_t* ctr;
};

/// Slots of the table of a row that looks for m positions with groups of G lanes: a power of two,
/// >= 2m, and above the m - 1 + G keys that the last batch can leave in it.
__host__ __device__ inline int32_t sample_slots(int32_t m, int32_t G) {
  int32_t t = SAMPLE_MIN_SLOTS;
  while (t < 2 * m || t < m + G)
    t <<= 1;
  return t;
}

/// Level 0: the distinct seeds (nullptr: every vertex) get local ids 0.. in list order.
__global__ void __launch_bounds__(SAMPLE_BLOCK)
    sample_seed_kernel(const int32_t* seeds, int32_t n0, int32_t* frontier, int32_t* local, int32_t* nodes) {
  for (long long i = blockIdx.x * (long long)SAMPLE_BLOCK + threadIdx.x; i < n0; i += (long long)gridDim.x * SAMPLE_BLOCK) {
    const int32_t v = seeds ? seeds[i] : (int32_t)i;
    frontier[i] = v;
    local[v] = (int32_t)i;
    if (nodes)
      nodes[i] = v;
  }
}

/// Per frontier row: min(d, k) entries, its class; per class the rows, and d per all-row.
__global__ void __launch_bounds__(SAMPLE_BLOCK)
    sample_count_kernel(const int32_t* ap, const int32_t* frontier, int32_t F, int32_t k, sample_rule_t rule,
                        int32_t* counts, unsigned char* cls, sample_counters_t* ctr) {
  const int lane = threadIdx.x & 63;
  unsigned long long copied = 0;
  for (long long base = blockIdx.x * (long long)SAMPLE_BLOCK; base < F; base += (long long)gridDim.x * SAMPLE_BLOCK) {
    const long long i = base + threadIdx.x;
    const bool in = i < F;
    int c = SC_CLASSES;  // nobody's
    if (in) {
      const int32_t v = frontier[i];
      const int32_t d = ap[v + 1] - ap[v];
      const sample_plan_t plan = sample_plan(d, k);
      if (d == 0)
        c = SC_NONE;
      else if (plan.mode == SAMPLE_ALL)
        c = d <= rule.copy8 ? SC_COPY8 : d <= rule.copy64 ? SC_COPY64 : SC_COPY256;
      else {
        // an exclude row reads all d positions out: it weighs d / 2 >= m
        const long long w = plan.mode == SAMPLE_INCLUDE ? plan.m : (d + 1) / 2;
        c = w <= rule.pick8 ? SC_PICK8 : w <= rule.pick64 ? SC_PICK64 : SC_PICK256;
      }
      counts[i] = plan.mode == SAMPLE_ALL ? d : k;
      cls[i] = (unsigned char)c;
      if (plan.mode == SAMPLE_ALL)
        copied += (unsigned long long)d;
    }
    for (int q = 0; q < SC_CLASSES; ++q) {
      const unsigned long long mask = __ballot(c == q);
      if (lane == 0 && mask)
        atomicAdd(&ctr->rows[q], (unsigned)__popcll(mask));
    }
  }
  copied = wave_sum(copied);
  if (lane == 0 && copied)
    atomicAdd(&ctr->attempts, copied);
}

/// All-rows: every entry, G lanes per row.  `order[begin, begin + count)`: the class's frontier rows.
template <int G>
__global__ void __launch_bounds__(SAMPLE_BLOCK)
    sample_copy_kernel(const sample_args_t a, const int32_t* order, int32_t begin, int32_t count) {
  constexpr int GROUPS = SAMPLE_BLOCK / G;
  const int gl = threadIdx.x % G;
  for (long long r = blockIdx.x * (long long)GROUPS + threadIdx.x / G; r < count; r += (long long)gridDim.x * GROUPS) {
    const int32_t i = order[begin + r];
    const int32_t v = a.frontier[i];
    const int32_t lo = a.ap[v], d = a.ap[v + 1] - lo;
    const int32_t o = a.row_off[i], room = a.row_off[i + 1] - o;
    for (int32_t j = gl; j < d && j < room; j += G) {
      a.t_src[o + j] = a.first_local + i;
      a.t_entry[o + j] = lo + j;
      a.t_nbr[o + j] = a.aj[lo + j];
    }
  }
}

/// What one group of G lanes agrees on: a barrier for G = 256 (the workgroup is the group), LDS
/// ordering inside the wavefront otherwise.
template <int G>
__device__ __forceinline__ void sample_group_sync() {
  if constexpr (G == SAMPLE_BLOCK) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

/// Over the group's lanes in lane order: how many of lanes 0..gl hold `pred`, and how many in all.
/// `s_scan`: four words of LDS (G = 256 only; two barriers).
template <int G>
__device__ __forceinline__ void sample_group_scan(bool pred, int gl, int* s_scan, int& incl, int& total) {
  const unsigned long long b = __ballot(pred);
  const int lane = threadIdx.x & 63;
  if constexpr (G == 64) {
    incl = __popcll(b & ((2ull << lane) - 1));
    total = __popcll(b);
  } else if constexpr (G < 64) {
    const unsigned long long bits = (b >> (lane & ~(G - 1))) & ((1ull << G) - 1);
    incl = __popcll(bits & ((2ull << gl) - 1));
    total = __popcll(bits);
  } else {
    const int wave = threadIdx.x >> 6;
    if (lane == 0)
      s_scan[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int w = 0; w < SAMPLE_BLOCK / 64; ++w) {
      const int t = s_scan[w];
      if (w < wave)
        before += t;
      total += t;
    }
    incl = before + __popcll(b & ((2ull << lane) - 1));
    __syncthreads();
  }
}

__device__ __forceinline__ int32_t sample_hash(int32_t x, int shift) {
  return (int32_t)(((uint32_t)x * 2654435761u) >> shift);
}

/**
 * @brief The picker: one group of G lanes per row that draws.  A batch is G attempts, lane l the
 * attempt a0 + l.  Every candidate goes into the row's LDS table (open addressing, linear probing:
 * key = position, att = the smallest attempt that named it, by atomicMin), so whether an attempt was
 * a first occurrence is a property of the table, not of the order in which lanes arrived.  The first
 * occurrences of a batch are counted in lane (= attempt) order: the batch in which the m-th distinct
 * position appears gives A exactly, and the positions of S are the keys with att < A.  Include:
 * later keys are freed, the table is sorted (bitonic, free slots last) and its first m keys leave in
 * order.  Exclude (d < 2048): the row is read out in order and the members of S are skipped.
 * Dynamic LDS: 2 * slots words for each of the workgroup's first `groups` groups.
 */
template <int G>
__global__ void __launch_bounds__(SAMPLE_BLOCK)
    sample_pick_kernel(const sample_args_t a, const int32_t* order, int32_t begin, int32_t count, int32_t slots,
                       int groups) {
  extern __shared__ int32_t s_table[];
  __shared__ int s_scan[SAMPLE_BLOCK / 64];
  __shared__ int32_t s_A;
  const int group = threadIdx.x / G, gl = threadIdx.x % G;
  const int lane = threadIdx.x & 63;
  const bool owns = group < groups;  // lanes that only fill the last wavefront have no table
  int32_t* key = s_table + (long long)(owns ? group : 0) * 2 * slots;
  int32_t* att = key + slots;
  unsigned long long attempts = 0;
  bool failed = false;
  for (long long r0 = blockIdx.x * (long long)groups; r0 < count; r0 += (long long)gridDim.x * groups) {
    const long long r = r0 + group;
    const bool live = owns && r < count;
    int32_t i = 0, v = 0, lo = 0, d = 0, o = 0, room = 0;
    if (live) {
      i = order[begin + r];
      v = a.frontier[i];
      lo = a.ap[v];
      d = a.ap[v + 1] - lo;
      o = a.row_off[i];
      room = a.row_off[i + 1] - o;
    }
    const sample_plan_t plan = sample_plan(d, a.k);
    const int32_t m = live ? (int32_t)plan.m : 0;
    int32_t T = sample_slots(m, G);
    bool done = !live || m == 0;
    if (T > slots) {  // the host sized the tables for the class's largest m
      T = SAMPLE_MIN_SLOTS;
      failed = live;
      done = true;
    }
    const int shift = 32 - (31 - __clz(T));
    for (int32_t j = gl; owns && j < T; j += G) {
      key[j] = SAMPLE_EMPTY;
      att[j] = INT32_MAX;
    }
    sample_group_sync<G>();

    const long long bound = sample_attempt_bound(m);
    const unsigned long long stream = walk_stream(a.seed, (unsigned long long)v);
    int32_t have = 0, A = 0;
    for (long long a0 = 0;; a0 += G) {
      if constexpr (G == SAMPLE_BLOCK) {
        if (done)
          break;
      } else {
        if (__ballot(!done) == 0)
          break;
      }
      const long long at = a0 + gl;
      int32_t slot = -1;
      if (!done && at < bound) {
        const int32_t x = (int32_t)walk_pick_uniform(walk_draw(stream, a.hop, (unsigned long long)at), d);
        int32_t s = sample_hash(x, shift);
        for (int32_t probes = 0; probes < T; ++probes) {
          const int32_t cur = atomicCAS(&key[s], SAMPLE_EMPTY, x);
          if (cur == SAMPLE_EMPTY || cur == x) {
            slot = s;
            break;
          }
          s = (s + 1) & (T - 1);
        }
        if (slot >= 0)
          atomicMin(&att[slot], (int32_t)at);
        else
          failed = true;
      }
      sample_group_sync<G>();
      const bool first = slot >= 0 && att[slot] == (int32_t)at;
      int incl, total;
      sample_group_scan<G>(first, gl, s_scan, incl, total);
      const int32_t need = m - have;
      const bool last = !done && total >= need;
      const bool hit = last && first && incl == need;  // the attempt that completes S
      if constexpr (G == SAMPLE_BLOCK) {
        if (hit)
          s_A = (int32_t)at + 1;
        __syncthreads();
        if (last)
          A = s_A;
        __syncthreads();
      } else {
        unsigned long long hits = __ballot(hit);
        if constexpr (G < 64)
          hits = (hits >> (lane & ~(G - 1))) & ((1ull << (G & 63)) - 1);
        if (last)
          A = (int32_t)a0 + (int32_t)__ffsll((long long)hits);
      }
      if (!done) {
        if (last) {
          done = true;
        } else {
          have += total;
          if (a0 + G >= bound) {  // cannot happen: see the header
            failed = true;
            done = true;
          }
        }
      }
    }
    if (gl == 0)
      attempts += (unsigned long long)A;

    if (A > 0 && plan.mode == SAMPLE_INCLUDE) {
      for (int32_t j = gl; j < T; j += G)
        if (key[j] != SAMPLE_EMPTY && att[j] >= A)
          key[j] = SAMPLE_EMPTY;
      sample_group_sync<G>();
      for (int32_t kk = 2; kk <= T; kk <<= 1)
        for (int32_t jj = kk >> 1; jj > 0; jj >>= 1) {
          for (int32_t p = gl; p < T; p += G) {
            const int32_t q = p ^ jj;
            if (q > p) {
              const int32_t x = key[p], y = key[q];
              if ((x > y) == ((p & kk) == 0)) {
                key[p] = y;
                key[q] = x;
              }
            }
          }
          sample_group_sync<G>();
        }
      for (int32_t j = gl; j < m && j < room; j += G) {
        const int32_t p = key[j];
        if (p < d) {  // a position of the row, were the table wrong
          a.t_src[o + j] = a.first_local + i;
          a.t_entry[o + j] = lo + p;
          a.t_nbr[o + j] = a.aj[lo + p];
        }
      }
    } else if (A > 0 && plan.mode == SAMPLE_EXCLUDE) {
      int32_t written = 0;
      for (int32_t p0 = 0; p0 < d; p0 += G) {
        const int32_t p = p0 + gl;
        bool keep = false;
        if (p < d) {
          keep = true;
          int32_t s = sample_hash(p, shift);
          for (int32_t probes = 0; probes < T; ++probes) {
            const int32_t cur = key[s];
            if (cur == SAMPLE_EMPTY)
              break;
            if (cur == p) {
              keep = att[s] >= A;
              break;
            }
            s = (s + 1) & (T - 1);
          }
        }
        int incl, total;
        sample_group_scan<G>(keep, gl, s_scan, incl, total);
        const int32_t j = written + incl - 1;
        if (keep && j < room) {
          a.t_src[o + j] = a.first_local + i;
          a.t_entry[o + j] = lo + p;
          a.t_nbr[o + j] = a.aj[lo + p];
        }
        written += total;
      }
    }
    sample_group_sync<G>();  // the tables are reused
  }
  attempts = wave_sum(attempts);
  if (lane == 0 && attempts)
    atomicAdd(&a.ctr->attempts, attempts);
  if (failed)
    a.ctr->failed = 1u;
}

/// Discovery: the lane that turns local[u] from -1 to -2 owns u and appends it to `claimed`.
__global__ void __launch_bounds__(SAMPLE_BLOCK)
    sample_claim_kernel(const int32_t* nbr, int32_t E, int32_t* local, int32_t* claimed, int32_t room,
                        sample_counters_t* ctr) {
  const int lane = threadIdx.x & 63;
  for (long long base = blockIdx.x * (long long)SAMPLE_BLOCK; base < E; base += (long long)gridDim.x * SAMPLE_BLOCK) {
    const long long e = base + threadIdx.x;
    int32_t u = -1;
    bool won = false;
    if (e < E) {
      u = nbr[e];
      won = local[u] == -1 && atomicCAS(&local[u], -1, -2) == -1;
    }
    const unsigned long long mask = __ballot(won);
    if (mask == 0)
      continue;
    unsigned at = 0;
    if (lane == 0)
      at = atomicAdd(&ctr->claimed, (unsigned)__popcll(mask));
    at = __shfl(at, 0, 64) + (unsigned)__popcll(mask & ((1ull << lane) - 1));
    if (won && at < (unsigned)room)
      claimed[at] = u;
  }
}

/// The sorted claims are the next level: local ids from `first_local` on.
__global__ void __launch_bounds__(SAMPLE_BLOCK)
    sample_assign_kernel(const int32_t* level, int32_t count, int32_t first_local, int32_t* local, int32_t* nodes) {
  for (long long i = blockIdx.x * (long long)SAMPLE_BLOCK + threadIdx.x; i < count; i += (long long)gridDim.x * SAMPLE_BLOCK) {
    local[level[i]] = first_local + (int32_t)i;
    if (nodes)
      nodes[first_local + i] = level[i];
  }
}

/// The hop's edges to the caller's arrays (each may be nullptr), neighbours as local ids.
__global__ void __launch_bounds__(SAMPLE_BLOCK)
    sample_fill_kernel(const int32_t* t_src, const int32_t* t_entry, const int32_t* t_nbr, int32_t E,
                       const int32_t* local, int32_t* src, int32_t* dst, int32_t* entry) {
  for (long long e = blockIdx.x * (long long)SAMPLE_BLOCK + threadIdx.x; e < E; e += (long long)gridDim.x * SAMPLE_BLOCK) {
    if (src)
      src[e] = t_src[e];
    if (entry)
      entry[e] = t_entry[e];
    if (dst)
      dst[e] = local[t_nbr[e]];
  }
}

}  // namespace kernels
}  // namespace hip
}  // namespace gunrock

#endif  // __HIPCC__

/*
 * essentials_amd.h -- C ABI of the MI355X-native frontier advance/filter engine.
 *
 * The reference (jdwapman/essentials) is a header-only C++ template library with
 * NO C ABI, FFI or plugin interface: its drop-in boundary is the template surface
 * under include/gunrock/ (this repository ships its own implementation of that
 * surface in include/gunrock/, against which the reference's bfs.hxx / sssp.hxx /
 * pr.hxx compile unchanged).  This header is therefore an ADDITION: the boundary
 * a non-C++ host (ctypes, cgo, JNI, ...) binds, with the engine's templates
 * pre-instantiated for the reference harnesses' types
 *     vertex_t = edge_t = int32_t, weight_t = float
 * (examples/algorithms/bfs/bfs.cu:16-18).  Each entry point names the reference
 * interface it stands for.  Conventions:
 *   - plain pointers and sizes only; every "d_" pointer is DEVICE memory owned by
 *     the caller (hipMalloc / a torch tensor's data_ptr), every "h_" pointer host;
 *   - return value 0 on success, a negative grx_status otherwise;
 *     grx_last_error() returns the message of the calling thread's last failure
 *     (the C++ surface throws gunrock::error::exception_t, reference error.hxx:21-46);
 *   - calls on one context are synchronous with respect to the host, like the
 *     reference's operators (advance/block_mapped.hxx:204);
 *   - one context per host thread; independent contexts do not share state
 *     (reference operators/batch/batch.hxx:69-74 relies on that).
 */
#ifndef ESSENTIALS_AMD_H
#define ESSENTIALS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRX_ABI_VERSION 1

typedef enum grx_status {
  GRX_OK = 0,
  GRX_ERR_INVALID_ARGUMENT = -1,
  GRX_ERR_RUNTIME = -2,      /* HIP / RCCL failure or an engine exception */
  GRX_ERR_UNSUPPORTED = -3,  /* variant not implemented (reference: "... not supported") */
  GRX_ERR_PEER = -4,         /* partitioned run: ANOTHER rank's superstep failed; every rank of the
                                job returns an error from the same superstep (the failing rank its own) */
  GRX_ERR_TIMEOUT = -5       /* partitioned run: the gathered counts of a superstep did not arrive
                                within GRX_PARTITIONED_TIMEOUT_MS (default 30 s) -- a peer is gone or
                                stuck.  The stream still holds the unfinished collective: the caller
                                should exit (not re-exec) without synchronising this context. */
} grx_status;

/* operators::load_balance_t (reference framework/operators/configs.hxx:31-39), same order */
typedef enum grx_load_balance {
  GRX_LB_THREAD_MAPPED = 0,
  GRX_LB_WARP_MAPPED = 1,
  GRX_LB_BLOCK_MAPPED = 2,
  GRX_LB_BUCKETING = 3,
  GRX_LB_MERGE_PATH = 4,
  GRX_LB_MERGE_PATH_V2 = 5,
  GRX_LB_WORK_STEALING = 6
} grx_load_balance;

/* operators::filter_algorithm_t (configs.hxx:73-78), same order */
typedef enum grx_filter_algorithm {
  GRX_FILTER_REMOVE = 0,
  GRX_FILTER_PREDICATED = 1,
  GRX_FILTER_COMPACT = 2,
  GRX_FILTER_BYPASS = 3
} grx_filter_algorithm;

/* operators::uniquify_algorithm_t (configs.hxx:80-85) */
typedef enum grx_uniquify_algorithm { GRX_UNIQUE = 0, GRX_UNIQUE_COPY = 1 } grx_uniquify_algorithm;

/* Built-in per-edge functors for grx_advance (device lambdas cannot cross a C ABI).
 * `state` / `iparam` are the functor's captured values. */
typedef enum grx_edge_op {
  GRX_OP_ALL = 0,        /* return true                                                     */
  GRX_OP_BFS = 1,        /* state: int32 depth[V]; it+1 < atomic::min(&depth[dst], it+1), it=iparam
                            (reference algorithms/bfs.hxx:92-114)                           */
  GRX_OP_SSSP = 2,       /* state: float dist[V]; d = dist[src]+w; d < atomic::min(&dist[dst], d)
                            (reference algorithms/sssp.hxx:110-124)                         */
  GRX_OP_COUNT_EDGE = 3, /* state: int32 calls[E]; atomic::add(&calls[edge],1); return (src+dst)%3==0 */
  GRX_OP_SUM_WEIGHT = 4  /* state: float acc[V]; atomic::add(&acc[dst], w); return false
                            (shape of reference algorithms/pr.hxx:140-146)                  */
} grx_edge_op;

/* Built-in predicates for grx_filter. */
typedef enum grx_vertex_op {
  GRX_PRED_ALL = 0,      /* return true                                                     */
  GRX_PRED_ODD = 1,      /* return v & 1                                                    */
  GRX_PRED_ONCE = 2,     /* state: int32 stamp[V]; stamp[v]==iparam ? false : (stamp[v]=iparam, true)
                            (reference algorithms/sssp.hxx:126-136)                         */
  GRX_PRED_COUNT = 3     /* state: int32 calls[V]; atomic::add(&calls[v],1); return v % 3 != 0 */
} grx_vertex_op;

typedef struct grx_context_s* grx_context_t; /* gcuda::multi_context_t, cuda/context.hxx:136-206 */
typedef struct grx_graph_s* grx_graph_t;     /* graph::graph_t over CSR, graph/build.hxx:26-36   */

/* enactor_properties_t (framework/enactor.hxx:31-54) + the engine's run-time switches */
typedef struct grx_options {
  int32_t load_balance;     /* grx_load_balance; default GRX_LB_BLOCK_MAPPED (what bfs.hxx spells) */
  int32_t holes_layout;     /* 1: one output slot per traversed edge, -1 holes (reference layout) */
  int32_t hub_threshold;    /* 0: default (256): longer lists are cut into chunks                */
  int32_t max_iterations;   /* 0: run to convergence                                              */
  float frontier_sizing_factor; /* 0: default 1.5 (enactor.hxx:36)                                */
  int32_t collect_kernel_time;  /* 1: event-time the advance kernels (adds two events per launch)  */
  int32_t chunk_edges;          /* 0: default (1024): edges per chunk of a hub list                */
  int32_t direction_optimized;  /* grx_bfs: 0 push every level (what bfs.hxx does); 1 pull the wide
                                   levels (advance_direction_t::backward).  grx_pagerank: 0 the push
                                   scatter of pr.hxx (one float atomic per edge); 1 the pull form (sums
                                   per destination over in-edges, no atomics).  Pulling needs in-edges:
                                   an undirected graph or grx_graph_build_in_edges                  */
  float do_alpha;               /* 0: default 4: pull when frontier edges > unexplored edges/alpha.
                                   grx_bfs with direction_optimized == 0 applies the same test
                                   (0: default 16) to its widest levels on a graph KNOWN to be
                                   symmetric (R-MAT symmetrised, a symmetric Matrix Market file, or
                                   verified by an earlier pull call); GRX_BFS_PULL=0 never pulls    */
  float do_beta;                /* 0: default 24: push again when frontier vertices < |V| / beta     */
  int32_t chunk_queue_limit;    /* test hook, 0: none. Caps the hub chunk queue to force the overflow
                                   path (hubs expanded in place)                                    */
  int32_t sssp_two_pass;        /* grx_sssp: 0 one pass -- the relax functor keeps exactly one copy of an
                                   improved vertex per round (one 64-bit atomic min on distance | round
                                   while the search runs; d_distances is written when it ends); 1 the
                                   reference client's formulation, advance + bypass filter with its racy
                                   stamp test (algorithms/sssp.hxx:110-144).  Same distances either way */
  int32_t call_every_edge;      /* grx_bfs push: 0 the search names its settled destinations (vertices that
                                   have a depth) and the engine skips the functor call for an edge into one
                                   (gunrock/framework/operators/settled.hxx; wide block_mapped levels);
                                   1 the functor is called for every edge, which is all the engine can do
                                   for the unchanged bfs.hxx.  Same depths either way                  */
} grx_options;

/* What enact() reports (framework/enactor.hxx:243-254 returns ms only; the rest is the
 * stats block util/info.hxx:36-71 names but never implemented). */
typedef struct grx_stats {
  float elapsed_ms;            /* device-event time around the BSP loop only           */
  float advance_kernel_ms;     /* sum of advance kernel durations (collect_kernel_time) */
  int32_t iterations;          /* loop() calls                                         */
  int32_t advance_launches;    /* advance kernel launches timed                        */
  int64_t vertices_reached;    /* BFS/SSSP: labels != unreached                        */
  int64_t edges_traversed;     /* BFS/SSSP: sum of out-degrees of reached vertices     */
  int32_t levels_recorded;     /* min(iterations, 64)                                  */
  int32_t pull_iterations;     /* direction-optimised BFS: levels expanded by pulling   */
  int64_t frontier_slots[64];  /* input-frontier length of each iteration              */
  int64_t edges_expanded;      /* BFS/SSSP push: functor calls = sum over iterations of the input
                                  frontier's degrees (SSSP relaxes a vertex again whenever its
                                  distance improved: > edges_traversed)                   */
} grx_stats;

/* ---- library ------------------------------------------------------------- */
int grx_abi_version(void);
const char* grx_last_error(void);

/* ---- context: gcuda::multi_context_t(device[, stream]) ------------------- */
/* stream: a hipStream_t to run on (e.g. torch.cuda.current_stream().cuda_stream) or NULL
 * for a private non-blocking stream (reference cuda/context.hxx:75-87,163-177). */
int grx_context_create(int device, void* stream, grx_context_t* out);
int grx_context_destroy(grx_context_t ctx);
int grx_context_synchronize(grx_context_t ctx);
/* Order everything already enqueued on `other_stream` (a hipStream_t; NULL = the null stream)
 * before the context's NEXT work, on the device (event record + stream wait, no host wait).  A
 * context created without a stream runs on a private NON-BLOCKING stream, which is not ordered
 * after the null stream or after any other: a host that fills operands on its own stream (torch
 * tensor ops) calls this before handing them to an engine entry point.  Results need no such call:
 * the entry points return after the context's stream has drained (except the enqueue-only
 * grx_partitioned_step / grx_partitioned_level_bitmap, which are meant to share the host's stream). */
int grx_context_wait_stream(grx_context_t ctx, void* other_stream);
/* Plain copies between host and device memory ON THE CONTEXT'S STREAM, complete when the call
 * returns (the stream is drained).  For bindings without a HIP runtime of their own -- e.g. a
 * host-staged collective callback (grx_context_attach_collectives). */
int grx_copy_to_host(grx_context_t ctx, void* h_dst, const void* d_src, size_t bytes);
int grx_copy_to_device(grx_context_t ctx, void* d_dst, const void* h_src, size_t bytes);
/* Return every device block the engine parked for reuse (frontier buffers of finished runs, up to
 * 64 GiB per process) to the device.  The engine does so by itself before it reports an
 * out-of-memory; a host that shares the device with another allocator calls this when THAT one
 * runs short. */
int grx_trim_cache(void);
int grx_context_device_info(grx_context_t ctx, int32_t* compute_units, int32_t* wavefront_size,
                            int64_t* total_memory_bytes, char* name, size_t name_len);

/* ---- graph: graph::build::from_csr<device, view_t::csr> ------------------ */
/* Non-owning view over caller-owned device CSR arrays (graph/graph.hxx:159-168).  The arrays must
 * be complete when the handle is first used (synchronise the stream that produced them) and must
 * not change while it lives: the handle reduces and keeps the graph's largest degree. */
int grx_graph_from_device_csr(int32_t n_rows, int32_t n_cols, int32_t nnz,
                              const int32_t* d_row_offsets, const int32_t* d_col,
                              const float* d_val, grx_graph_t* out);
/* Owning device copy of host CSR arrays (format::csr_t<device>, formats/csr.hxx:25-77). */
int grx_graph_from_host_csr(int32_t n_rows, int32_t n_cols, int32_t nnz,
                            const int32_t* h_row_offsets, const int32_t* h_col,
                            const float* h_val, grx_graph_t* out);
/* Matrix Market file -> owning device CSR (io/matrix_market.hxx:99-240 + csr.hxx:79-157). */
int grx_graph_from_mtx(const char* path, grx_graph_t* out);
/* ".csr" binary cache (formats/csr.hxx:159-236). */
int grx_graph_from_csr_file(const char* path, grx_graph_t* out);
int grx_graph_write_csr_file(grx_graph_t g, const char* path);
/* Synthetic R-MAT (no reference counterpart; spec in DESIGN.md, oracle in oracle/grx_oracle.c):
 * 2^scale vertices, edge_factor*2^scale generated pairs, loader-style symmetrisation when
 * symmetrize != 0, weights 1.0f when weight_seed == 0 else integers in [1,64]. Built on the GPU. */
int grx_graph_rmat(grx_context_t ctx, uint32_t scale, uint32_t edge_factor, uint64_t seed,
                   uint64_t weight_seed, int symmetrize, grx_graph_t* out);
/* Copy of `g` whose neighbour lists are sorted by column id (duplicates adjacent, weights carried
 * along): the layout a column-major-sorted Matrix Market file (SuiteSparse convention) gets from
 * the reference's stable row sort (formats/csr.hxx:119-147).  The R-MAT generator above keeps the
 * EMISSION order inside a row (an unsorted edge-list file); this utility produces the other
 * common layout of the same graph. */
int grx_graph_sorted_rows(grx_context_t ctx, grx_graph_t g, grx_graph_t* out);
/* Owning copy of `g` as a SIMPLE graph: self loops dropped, repeated entries of a row kept once
 * (weight: the smallest of the repeats, so that SSSP distances are unchanged), rows sorted by
 * column.  A symmetric input gives a symmetric output, and the copy carries the input's symmetry
 * verdict when it is known.  The layout on which grx_kcore returns the textbook core numbers and
 * grx_tc's per-vertex counts equal the reference's. */
int grx_graph_simple(grx_context_t ctx, grx_graph_t g, grx_graph_t* out);
/* Build and attach the in-edge (transpose / csc) arrays of a DIRECTED graph so that pull advances
 * (grx_options.direction_optimized) can walk in-neighbours; graphs without them are taken to be
 * undirected (symmetric CSR = its own transpose).  Reference counterpart: the csc view of
 * graph::build::from_csr (graph/detail/build.hxx:96-113), which it cannot combine with csr. */
int grx_graph_build_in_edges(grx_context_t ctx, grx_graph_t g);
/* Hot-first numbering (engine data layout, no reference counterpart; the reference's views keep
 * the loader's numbering, graph/build.hxx:26-52).  grx_bfs / grx_sssp run on a copy of the graph
 * whose vertices are renumbered in descending order of out-degree
 * (include/gunrock/graph/reorder.hxx) and deliver their labels in the CALLER's numbering: sources
 * in, labels out, nothing else changes at this boundary.  The copy (a second CSR + 8 bytes per
 * vertex) is built on the first traversal of a square graph of >= 2^16 vertices and >= 2^20 edges
 * without attached in-edges (GRX_HOT_FIRST=0/1 overrides the size rule); enable = 1 builds it now
 * for any square graph, enable = 0 drops it and keeps this handle on its own numbering.  The
 * options that stand for the unchanged reference clients (call_every_edge, sssp_two_pass) and the
 * holes layout always run on the caller's numbering. */
int grx_graph_hot_first(grx_context_t ctx, grx_graph_t g, int enable);
int grx_graph_destroy(grx_graph_t g);
int grx_graph_info(grx_graph_t g, int32_t* n_rows, int32_t* n_cols, int64_t* nnz,
                   const int32_t** d_row_offsets, const int32_t** d_col, const float** d_val);
int grx_graph_copy_to_host(grx_graph_t g, int32_t* h_row_offsets, int32_t* h_col, float* h_val);

/* ---- algorithms: gunrock::{bfs,sssp,pr}::run ------------------------------ */
void grx_default_options(grx_options* opt);
/* bfs::run(G, source, distances, predecessors, context)  algorithms/bfs.hxx:151-176.
 * d_distances: int32[V] out (INT32_MAX = unreached). d_predecessors: unused by the reference
 * ("@todo", bfs.hxx:28), may be NULL, never written: grx_bfs_predecessors derives the parents from
 * the depths this call delivers. */
int grx_bfs(grx_context_t ctx, grx_graph_t g, int32_t source, int32_t* d_distances,
            int32_t* d_predecessors, const grx_options* opt, grx_stats* stats);
/* sssp::run(G, source, distances, predecessors, context)  algorithms/sssp.hxx:155-185.
 * d_distances: float[V] out (FLT_MAX = unreached).  d_predecessors: as for grx_bfs, may be NULL,
 * never written: grx_sssp_predecessors derives the tree from the distances this call delivers.
 * On a graph KNOWN to be its own transpose with equal weights in both directions (grx_graph_rmat
 * with symmetrize, grx_graph_from_mtx on a symmetric file; no check is ever run for this) the wide
 * rounds that follow a near / far selection are pulled over a copy of the rows sorted by ascending
 * weight: 8 bytes per edge and 4 per vertex on the handle, built by the first such call outside its
 * timed part, released with the handle; not built when a weight is NaN or the graph has fewer edges
 * than a selection needs, and a build that fails leaves the call pushing as before.  Same distances;
 * stats.pull_iterations counts the pulled rounds.  GRX_SSSP_PULL=0 never pulls,
 * GRX_SSSP_PULL_ALPHA (default 0.5; 0: every eligible round) sets the rule's factor. */
int grx_sssp(grx_context_t ctx, grx_graph_t g, int32_t source, float* d_distances,
             int32_t* d_predecessors, const grx_options* opt, grx_stats* stats);
/* pr::run(G, alpha, tol, p, context)  algorithms/pr.hxx:182-216.  d_p: float[V] out. */
int grx_pagerank(grx_context_t ctx, grx_graph_t g, float alpha, float tol, float* d_p,
                 const grx_options* opt, grx_stats* stats);
/* bc::run(G, source, bc_values) summed over a list of sources  algorithms/bc.hxx.
 * h_sources: HOST int32[n_sources] in the caller's numbering; NULL = every vertex 0..V-1
 * (n_sources must then be 0).  d_bc: float[V] out, overwritten.  Needs in-edges: an undirected
 * graph or grx_graph_build_in_edges (GRX_ERR_UNSUPPORTED otherwise, as for pull PageRank).
 * bc[v] = 0.5 * sum over sources s of delta_s(v) (Brandes, hop counts, edge weights ignored);
 * the same call on the same handle returns bit-identical values.  All of it is float32 and every
 * term is non-negative: the relative error of bc[v] grows with the number of roundings on the
 * paths through v (the longest sums and the depth), not with max |bc|, and a vertex on no shortest
 * path gets +0.  Shortest-path counts above FLT_MAX, and reciprocals of counts below the normal
 * range (more than 2^126 paths between two vertices), are outside the contract -- as they are for
 * the reference's float atomics.  opt: read as grx_bfs reads it
 * for the depth search; max_iterations must be 0.  stats: elapsed_ms (the whole call),
 * iterations (BFS levels), vertices_reached and edges_traversed, each summed over sources. */
int grx_bc(grx_context_t ctx, grx_graph_t g, const int32_t* h_sources, int32_t n_sources,
           float* d_bc, const grx_options* opt, grx_stats* stats);
/* tc::run(G, reduce_all_triangles, vertex_triangles_count, &total)  algorithms/tc.hxx
 * Counts the triangles of the SIMPLE UNDIRECTED graph under the CSR: self loops are ignored,
 * repeated entries of a row count once, and row order does not matter (unsorted rows give the
 * same answer).  d_vertex_triangles: device int64[V] out, overwritten with the number of triangles
 * that contain each vertex (the caller's numbering); NULL = the total only.  h_triangles: HOST
 * out, the number of DISTINCT triangles T (the reference's total_triangles_count is the sum of
 * its per-vertex counts, 3 * T); NULL = per-vertex counts only.  At least one of the two outputs
 * must be non-NULL (GRX_ERR_INVALID_ARGUMENT otherwise).  On a graph whose rows are sorted and
 * free of repeats (self loops allowed) the per-vertex counts equal the reference's
 * vertex_triangles_count, and its total equals 3 * T; the per-vertex counts are 64-bit on purpose
 * (the reference's int32 can overflow on hubs).  Undirected input only: n_rows != n_cols is
 * GRX_ERR_INVALID_ARGUMENT; a handle with in-edges attached, or a CSR that is not its own
 * transpose (verified once when unknown), is GRX_ERR_UNSUPPORTED.  opt may be NULL; only
 * collect_kernel_time is read.  stats may be NULL; set: elapsed_ms (the whole call),
 * advance_kernel_ms (the counting kernels alone, when collect_kernel_time is set), iterations (1),
 * edges_traversed (oriented edges = simple undirected edges that are not self loops) and
 * edges_expanded (intersection work: neighbour-list entries probed).  The call leaves no state on
 * the handle but the symmetry verdict (no hot-first copy is built); its workspace is released
 * when it returns.  Same call, same results (integer sums). */
int grx_tc(grx_context_t ctx, grx_graph_t g, int64_t* d_vertex_triangles,
           uint64_t* h_triangles, const grx_options* opt, grx_stats* stats);
/* kcore::run(G, k_cores)  algorithms/kcore.hxx
 * Core numbers by peeling THE CSR AS IT IS GIVEN, every entry counting: the degree of v is the
 * length of row v, a repeated entry counts each time it appears, and a self loop counts as the one
 * entry it is and is never taken away before its vertex leaves.  core[v] is the value of k at which
 * v leaves when, for k = 1, 2, ..., vertices of remaining degree <= k are removed until none is
 * left, each removal lowering the remaining degree of the vertex named by every entry of the
 * removed row.  That is what kcore.hxx and the reference's kcore_cpu.hxx compute, so on any
 * symmetric CSR d_core equals the reference's k_cores; on a simple graph (no repeats, no self
 * loops) it is the textbook core number.  The result does not depend on the order of removals or of
 * a row's entries: the same call returns identical values.  The call does NOT deduplicate (the
 * R-MAT generator emits a multigraph whose degeneracy by entries is about twice the simple graph's):
 * a caller who wants the simple graph's core numbers passes grx_graph_simple of the handle.
 * d_core: device int32[V] out, overwritten, the caller's numbering; a vertex with an empty row gets
 * 0.  h_degeneracy: HOST out, the largest core number (0 for a graph without entries).  At least
 * one of the two must be non-NULL (GRX_ERR_INVALID_ARGUMENT otherwise); with d_core == NULL the call
 * uses a workspace of its own.  Undirected input only: n_rows != n_cols is
 * GRX_ERR_INVALID_ARGUMENT; a handle with in-edges attached, or a CSR that is not its own transpose
 * (verified once when unknown), is GRX_ERR_UNSUPPORTED.  opt may be NULL; only collect_kernel_time
 * is read, and max_iterations != 0 is GRX_ERR_INVALID_ARGUMENT.  stats may be NULL; set: elapsed_ms
 * (the whole call), advance_kernel_ms (the peeling kernels, batch by batch, when
 * collect_kernel_time is set), advance_launches (kernel launches of the peel), iterations (the
 * number of DISTINCT NON-ZERO core values: defined by the answer, not by the schedule),
 * vertices_reached (vertices with a non-empty row), edges_traversed = edges_expanded (row entries
 * walked: each row is walked once, when its vertex leaves, so this equals nnz).  The call leaves no
 * state on the handle but the symmetry verdict (no hot-first copy is built or used); its workspace
 * is released when it returns. */
int grx_kcore(grx_context_t ctx, grx_graph_t g, int32_t* d_core, int32_t* h_degeneracy,
              const grx_options* opt, grx_stats* stats);
/* Graph colouring (the reference's color.hxx hands out two fresh colours per filter pass by
 * rand()-style priorities, so no two runs agree; this is not a port of it).
 * GREEDY COLOURING IN LARGEST-DEGREE-FIRST ORDER: a function of the CSR arrays alone, and the same
 * call returns bit-identical results.  deg(v) is the length of row v as given (a repeated entry
 * counts each time, a self loop once) and
 *     key(v) = ((uint64_t)deg(v) << 32) | fmix32(v)
 * where fmix32 is the 32-bit finaliser on the unsigned vertex id (h ^= h >> 16; h *= 0x85ebca6b;
 * h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16): a bijection, so keys are distinct, the order is
 * strict and total and there is no tie to break.  u PRECEDES v when u != v, u appears in row v and
 * key(u) > key(v).  color[v] is the smallest integer >= 0 that is not the colour of a vertex that
 * precedes v: exactly what sequential greedy colouring gives when it takes the vertices in
 * descending key.  Self loops never constrain, a repeated entry constrains once, a vertex with an
 * empty row gets 0; hence color[v] <= (distinct predecessors of v) <= deg(v), and adjacent vertices
 * never share a colour.
 * d_colors: device int32[V] out, overwritten, the caller's numbering.  h_num_colors: HOST out,
 * 1 + the largest colour, 0 when V == 0.  At least one of the two must be non-NULL
 * (GRX_ERR_INVALID_ARGUMENT otherwise); with d_colors == NULL the call works on an array of its own.
 * Undirected input only: n_rows != n_cols is GRX_ERR_INVALID_ARGUMENT; a handle with in-edges
 * attached, or a CSR that is not its own transpose (verified once when unknown), is
 * GRX_ERR_UNSUPPORTED (a coloured vertex tells the vertices it precedes through its own row, which
 * needs every edge stored from both ends).  V == 0 is GRX_OK with nothing written.  opt may be NULL;
 * only collect_kernel_time is read, and max_iterations != 0 is GRX_ERR_INVALID_ARGUMENT.
 * Method: Jones-Plassmann, data-driven.  One pass counts, per vertex, the entries of its row that
 * name a predecessor; the vertices without any form generation 1.  A generation's vertices take
 * their colours (a 64-bit mask of the predecessors' colours; when it is full, and for rows above
 * GRX_COLOR_BIG_ROW entries (default 4096), a bitmap of GRX_COLOR_MEX_WINDOW colours (default and
 * at most 2048) that moves up until a window has a gap) and lower the count of every vertex they
 * precede; the decrement that reaches 0 puts that vertex into the next generation.  Generations of
 * at most 1024 vertices and GRX_COLOR_NARROW_EDGES entries (default 16384; 0 = never) run inside one
 * workgroup without the host.
 * stats may be NULL; set: elapsed_ms (the whole call), advance_kernel_ms (the kernels, batch by
 * batch, when collect_kernel_time is set), advance_launches (kernel launches), iterations (the
 * DEPTH OF THE PRIORITY DAG: depth(v) = 1 + the largest depth of a predecessor, 1 without one;
 * iterations = the largest depth, 0 for V == 0 -- defined by the answer, not by how generations were
 * batched), vertices_reached (vertices with a non-empty row), edges_traversed = nnz, edges_expanded
 * = 2 * nnz (each entry is classified once when predecessors are counted and once when its row's
 * vertex is coloured; re-reads inside one colouring do not count).  The call builds and uses no
 * hot-first copy, leaves no state on the handle but the symmetry verdict and releases its workspace
 * when it returns. */
int grx_color(grx_context_t ctx, grx_graph_t g, int32_t* d_colors, int32_t* h_num_colors,
              const grx_options* opt, grx_stats* stats);
/* Connected components (no reference counterpart: the reference has no such algorithm).
 * Every row entry (u, v) joins u and v, whatever its direction: on a symmetric CSR the result is
 * the connected components, on a directed one the WEAKLY connected components.  Self loops and
 * repeated entries change nothing.  d_component: device int32[V] out, overwritten;
 * d_component[v] is the SMALLEST VERTEX ID, in the caller's numbering, of the component that holds
 * v.  Hence d_component[v] <= v, v is its component's representative iff d_component[v] == v, and
 * the result is a function of the graph alone: not of the schedule, the order of a row's entries,
 * the sampling below or a hot-first copy.  The same call returns bit-identical values.
 * h_components: HOST out, the number of components (an isolated vertex is one).  At least one of
 * the two must be non-NULL (GRX_ERR_INVALID_ARGUMENT otherwise); with d_component == NULL the call
 * uses a workspace of its own.  A directed CSR is supported and needs no in-edges (attached ones
 * are ignored); n_rows != n_cols is GRX_ERR_INVALID_ARGUMENT; V == 0 is GRX_OK with
 * *h_components = 0 and nothing written.  opt may be NULL; only collect_kernel_time is read, and
 * max_iterations != 0 is GRX_ERR_INVALID_ARGUMENT.
 * Method: Afforest -- lock-free union-find on d_component itself (the larger root is hooked under
 * the smaller by a 32-bit compare-and-swap, so a tree's root is its smallest member), two neighbour
 * rounds (round r hooks every vertex to entry r of its row; GRX_CC_SAMPLE_ROUNDS = 0..8 overrides,
 * 0 = hook every entry), then a remainder pass over the other entries that LEAVES THE ROWS OF THE
 * MOST FREQUENT COMPONENT UNREAD.  That skip is sound only when every edge is stored from both
 * ends, so it is taken only when the handle's symmetry verdict is already "symmetric" (R-MAT with
 * symmetrize, symmetric Matrix Market files, handles another call has verified) and no in-edges
 * are attached; the call does not start the verification itself.  Otherwise every row is walked in
 * full.  stats may be NULL; set: elapsed_ms (the whole call), advance_kernel_ms (the kernels alone,
 * when collect_kernel_time is set), advance_launches (kernel launches), iterations (passes over
 * neighbour positions: the neighbour rounds + the remainder pass -- defined by the schedule, not
 * by the answer), vertices_reached (V - components: vertices that are not their component's
 * representative), edges_traversed = edges_expanded (row entries the hooking kernels read: nnz
 * when every row is walked, a small part of it when the skip applies; with the skip a vertex that
 * joins the picked component while the remainder pass runs may or may not have its row read, so
 * this figure can differ by a few rows between calls -- the labels cannot).  The call runs on the
 * caller's CSR as given, builds and uses no hot-first copy, leaves nothing on the handle and
 * releases its workspace when it returns. */
int grx_cc(grx_context_t ctx, grx_graph_t g, int32_t* d_component, int64_t* h_components,
           const grx_options* opt, grx_stats* stats);
/* Strongly connected components (no reference counterpart: the reference has no such algorithm).
 * u and v share a component iff each reaches the other along row entries.  d_component: device
 * int32[V] out, overwritten; d_component[v] is the SMALLEST VERTEX ID, in the caller's numbering, of
 * the strongly connected component that holds v: the convention of grx_cc, so the two compose.
 * Hence d_component[v] <= v, v is its component's representative iff d_component[v] == v, and the
 * result is a function of the CSR alone: not of the schedule, the pivots, the order of a row's
 * entries or a hot-first copy.  The same call returns bit-identical values.  Self loops and repeated
 * entries change nothing; a vertex on no cycle is a component of one.  h_components: HOST out, the
 * number of components.  At least one of the two must be non-NULL (GRX_ERR_INVALID_ARGUMENT
 * otherwise); with d_component == NULL the call works on an array of its own.  n_rows != n_cols is
 * GRX_ERR_INVALID_ARGUMENT; V == 0 is GRX_OK with *h_components = 0 and nothing written.  opt may be
 * NULL; only collect_kernel_time is read, and max_iterations != 0 is GRX_ERR_INVALID_ARGUMENT.
 * Which edges: with in-edges attached (grx_graph_build_in_edges) the call walks both arrays.
 * Without them, when the handle's verdict is "symmetric" (an unknown one is verified first, as
 * grx_bc and pull PageRank do), every edge runs both ways and the answer is grx_cc's: the call
 * returns grx_cc on the same arguments, stats included.  Without in-edges and asymmetric:
 * GRX_ERR_UNSUPPORTED, and the message names grx_graph_build_in_edges.
 * Method: forward-backward with trimming, all regions at once, on the generation queue of
 * grx_kcore.  A region is a set of unfinished vertices known to be a union of whole components (at
 * the start: everything); an entry is alive when it is no self loop and both ends are unfinished and
 * in one region.  Trimming: a vertex without an alive out-entry or in-entry is a component of one;
 * it leaves, its rows lower its neighbours' counts, and whoever reaches 0 follows.  A round: every
 * region picks the vertex of largest key(v) = (min(alive_out(v) * alive_in(v), 2^32 - 1) << 32) |
 * fmix32(v) as its pivot (fmix32: grx_color's hash), the pivots' forward reach FW over the out-rows
 * and backward reach BW over the in-rows are marked, FW n BW is the pivot's component and FW \ BW,
 * BW \ FW and the rest are the regions of the next round, which are counted and trimmed again.
 * Rows above GRX_SCC_BIG_ROW entries (default 4096) are walked by the whole grid; generations of at
 * most 1024 vertices and GRX_SCC_NARROW_EDGES entries (default 16384; 0 = never) run inside one
 * workgroup without the host; GRX_SCC_TRIM = 0 switches trimming off (singletons are then found as
 * pivots; for tests).  More than V rounds is GRX_ERR_RUNTIME.
 * stats may be NULL; set: elapsed_ms (the whole call), advance_kernel_ms (the kernels, batch by
 * batch, when collect_kernel_time is set), advance_launches (kernel launches), iterations (the
 * forward-backward rounds run -- defined by the schedule; 0 when trimming finished everything),
 * vertices_reached (V - components), edges_traversed = edges_expanded (row entries of either array
 * read by the counting, trimming and reach kernels: at most 2 * nnz * (2 * iterations + 2)).  The
 * call runs on the caller's CSR as given, builds and uses no hot-first copy, leaves nothing on the
 * handle but the symmetry verdict and releases its workspace when it returns. */
int grx_scc(grx_context_t ctx, grx_graph_t g, int32_t* d_component, int64_t* h_components,
            const grx_options* opt, grx_stats* stats);
/* Community detection (no reference counterpart: the reference has no such algorithm).
 * SEMI-SYNCHRONOUS LABEL PROPAGATION (Cordasco, Gargano 2010; the method behind
 * networkx.community.label_propagation_communities) over the colour classes of grx_color: a
 * function of the CSR arrays alone, and the same call returns bit-identical values.  The float
 * values are ignored (as grx_bc ignores them), a repeated entry counts each time it appears, a self
 * loop is ignored and the order of a row's entries does not matter.  color[] is exactly what
 * grx_color returns for the handle.  Start: label[v] = v.  A SWEEP takes the colour classes in order
 * c = 0, 1, ..., num_colors - 1; every vertex v of a class decides at once, from the labels as they
 * stand when its class begins: count(l) is the number of entries (v, u) of row v with u != v and
 * label[u] == l, and best the largest count.  v keeps its label when its row has no entry other than
 * self loops, or when count(label[v]) == best; otherwise it takes, among the labels with count ==
 * best, the one of smallest fmix32(l) (grx_color's hash: a bijection, so there is no tie left).
 * Vertices of one class are never adjacent, so deciding at once equals deciding one by one in any
 * order.  The call stops after the first sweep that changes no label, or after opt->max_iterations
 * sweeps when that is not 0.  A vertex that moves from a to b has count(b) > count(a), which on a
 * symmetric CSR raises the number of entries whose ends share a label by 2 * (count(b) - count(a));
 * that number is at most nnz, so at most nnz / 2 sweeps change anything, and running more than
 * nnz / 2 + 2 sweeps is GRX_ERR_RUNTIME (it cannot happen unless the kernels are wrong).
 * d_community: device int32[V] out, overwritten; d_community[v] is the SMALLEST VERTEX ID that ends
 * with the same label as v: the convention of grx_cc, so d_community[v] <= v and v names its
 * community iff d_community[v] == v.  h_communities: HOST out, the number of distinct final labels
 * (an isolated vertex is a community of its own).  h_modularity: HOST out, what grx_modularity
 * returns for d_community.  At least one of the three must be non-NULL (GRX_ERR_INVALID_ARGUMENT
 * otherwise); with d_community == NULL the call works on an array of its own.  NULL ctx or g,
 * n_rows != n_cols and max_iterations < 0 are GRX_ERR_INVALID_ARGUMENT; a handle with in-edges
 * attached, or a CSR that is not its own transpose (verified once when unknown), is
 * GRX_ERR_UNSUPPORTED.  V == 0 is GRX_OK with *h_communities = 0, *h_modularity = 0.0 and nothing
 * written.  opt may be NULL; only collect_kernel_time and max_iterations are read.
 * Method: the vertices are sorted once by (colour, row-length bin).  A decision gathers label[u]
 * per entry into a table of (label, count) in LDS -- open addressing, compare-and-swap on the key,
 * integer add on the count, at most half full: 8 lanes and 64 slots per row up to 32 entries, a
 * wavefront and 512 slots up to 256, a workgroup of 256 threads and two slots per entry up to
 * GRX_LPA_BIG_ROW entries (default 4096), and above that, as a whole row, a workgroup of 1024
 * threads with the largest table the device's LDS holds (GRX_LPA_LDS_SLOTS lowers it; for tests).
 * A row with more distinct labels than half that table -- a hub in the first sweep -- is decided
 * again by the same workgroup code on a table of two slots per entry in global memory.  A dirty
 * byte per vertex: a vertex decides only while its byte is set, and a vertex that changes its label
 * sets the byte of every other vertex in its row; a vertex none of whose neighbours changed would
 * decide the same, so labels and sweeps are those of the definition (GRX_LPA_ALL_ROWS = 1 decides
 * every vertex every sweep; for tests).  A sweep is one launch per non-empty bin of every class,
 * except that consecutive classes of at most 1024 vertices and GRX_LPA_NARROW_EDGES entries (default
 * 16384; 0 = never) run inside one workgroup; one hand-off per sweep carries its change count.
 * stats may be NULL; set: elapsed_ms (the whole call, the colouring included), advance_kernel_ms
 * (the call's own kernels, batch by batch, when collect_kernel_time is set; the colouring's are not
 * in it), advance_launches (the call's own kernel launches), iterations (the sweeps run, counting
 * the last one, which changed nothing), levels_recorded = min(iterations, 64), frontier_slots[t]
 * (the labels that changed in sweep t + 1; never microseconds, with or without
 * collect_kernel_time), vertices_reached (V - communities), edges_traversed = nnz, edges_expanded
 * (the row entries of the deciding vertices plus those of the vertices that changed, whose rows are
 * walked again to set the dirty bytes; iterations * nnz under GRX_LPA_ALL_ROWS; re-reads inside one
 * decision do not count).  The colouring's own stats are not reported.  The call builds and uses no
 * hot-first copy, leaves no state on the handle but the symmetry verdict and releases its workspace
 * when it returns: 13 bytes per vertex (colours 4, sort keys 4, class lists 4, dirty bytes 1), 4
 * more each when d_community is NULL and when h_modularity is asked for, the sort's temporary
 * storage while it runs, and 16 bytes per entry of the rows above GRX_LPA_BIG_ROW of the one class
 * that has most of them. */
int grx_lpa(grx_context_t ctx, grx_graph_t g, int32_t* d_community, int64_t* h_communities,
            double* h_modularity, const grx_options* opt, grx_stats* stats);
/* Modularity of any labelling, in exact integers.  d_label: device int32[V] with values in [0, V)
 * (the outputs of grx_lpa, grx_cc and grx_scc qualify); a label outside that range is found by a
 * device pass before anything is reported and is GRX_ERR_INVALID_ARGUMENT.  E = nnz: every entry
 * counts as given, self loops and repeats included, and the float values are ignored.  I is the
 * number of entries whose two ends carry the same label, tot(l) the sum of the row lengths of the
 * vertices labelled l and S the sum over l of tot(l)^2 (S <= E^2 < 2^62).  Then
 *     *h_modularity = (double)I / (double)E - (double)S / ((double)E * (double)E)
 * computed on the host in exactly this form, 0.0 when E == 0.  h_inside_entries receives I and
 * h_degree_squares S; each of the three may be NULL, at least one must not be.  On a simple
 * symmetric graph without self loops this is networkx.community.modularity at resolution 1.  A
 * directed CSR is accepted (no in-edges are needed, attached ones are ignored), but the value is
 * then NOT the standard directed modularity, which multiplies out-degree by in-degree sums.
 * n_rows != n_cols is GRX_ERR_INVALID_ARGUMENT.  Only integer atomics and integer reductions are
 * used, so results are bit-identical from call to call.  opt may be NULL; only collect_kernel_time
 * is read.  stats may be NULL; set: elapsed_ms, advance_kernel_ms, advance_launches, iterations = 1,
 * edges_traversed = edges_expanded = nnz.  Workspace: 4 bytes per vertex and 8 bytes per 2048
 * entries (the segments of long rows), released on return. */
int grx_modularity(grx_context_t ctx, grx_graph_t g, const int32_t* d_label, double* h_modularity,
                   int64_t* h_inside_entries, uint64_t* h_degree_squares, const grx_options* opt,
                   grx_stats* stats);
/* Community detection by MULTI-LEVEL MODULARITY OPTIMISATION (Louvain; Blondel et al. 2008), defined
 * in exact integers: a function of the CSR arrays alone, the same call returns bit-identical values,
 * and there is no float gain, no float atomic and no random order.  Resolution is fixed at 1; a
 * resolution parameter, Leiden refinement and directed modularity are out of scope.
 * Input: as grx_lpa, a square CSR that is its own transpose (verified once when unknown;
 * GRX_ERR_UNSUPPORTED otherwise, also with in-edges attached).  The float values are ignored.
 * E = nnz, k(v) is the row length, a repeated entry counts each time: the conventions of
 * grx_modularity, Q = I / E - S / E^2.
 * LEVEL GRAPH: n_L vertices, integer weights w(u, v) = w(v, u), k(v) = the sum of row v, the self
 * entry included.  Level 0 is the handle's CSR with weight 1 per entry, used in place.
 * PHASE: label[v] = v, tot[c] = k(c).  The vertices are coloured by grx_color on the level graph's
 * pattern CSR (above level 0: one entry per distinct pair, rows ascending by column, the self
 * entry present when its weight is positive).  A SWEEP takes the colour classes in order.  Every
 * vertex v of a class decides from label and tot AS THEY STAND WHEN ITS CLASS BEGINS: for every
 * label c carried by some entry (v, u) with u != v, k_vc is the sum of those entries' weights;
 * t(c) = tot[c], minus k(v) when c == label[v]; gain(c) = k_vc * E - k(v) * t(c) as int64 (both
 * products are below 2^62 because E < 2^31); gain(own) uses k_v,own, which may be 0.  v stays when
 * it has no entry other than self entries, or when no other label has gain > gain(own); otherwise
 * it takes the label of largest gain, among equal gains the one of smallest fmix32(c), c being the
 * level-local id.  When the class is done its moves are applied: label[v], tot[old] -= k(v),
 * tot[new] += k(v).  Two vertices of one class can interact through tot, so a sweep need not raise
 * the score: after each sweep N = I * E - S is evaluated in exact integers (I: the weight of the
 * entries whose two ends share a label, S: the sum of tot^2; both terms below 2^62).  A sweep with
 * no move ends the phase; a sweep with moves that leaves N <= N_before is UNDONE (label and tot
 * return to their state before it) and ends the phase.  N rises strictly with every kept sweep,
 * which bounds the sweeps.  There is no dirty-vertex rule: every vertex with a non-empty row
 * decides in every sweep.
 * AGGREGATION: if the phase kept no move the run ends.  Otherwise the communities become the
 * vertices of the next level, numbered by ascending smallest original vertex id; w'(a, b) is the
 * sum of w(u, v) over u in a and v in b, the self entry w'(a, a) holding the inside weight.  E and
 * N are unchanged by construction, and weights stay int32 because every weight is at most E.
 * STOP: when a phase keeps no move, or after opt->max_iterations phases when that is not 0; the
 * partition after t phases is then the result (a dendrogram cut).
 * d_community: device int32[V] out; each entry is the smallest original vertex id in the same final
 * community (the grx_cc / grx_lpa convention).  h_communities: HOST out.  h_modularity: HOST out,
 * exactly (double)I / (double)E - (double)S / ((double)E * (double)E) (0.0 when E == 0), bit-equal
 * to grx_modularity of d_community.  h_levels: HOST out, the phases run, counting the last one,
 * which keeps nothing.  At least one of the four must be non-NULL; with d_community == NULL the
 * call works on an array of its own.  NULL ctx or g, n_rows != n_cols and max_iterations < 0 are
 * GRX_ERR_INVALID_ARGUMENT.  V == 0 is GRX_OK with *h_communities = 0, *h_modularity = 0.0,
 * *h_levels = 0 and nothing written.  opt may be NULL; only collect_kernel_time and max_iterations
 * are read.
 * Method: the schedule and the tables of grx_lpa.  The vertices of a level are sorted once by
 * (colour, row-length bin); a decision gathers (label[u], w) per entry into a table of (community,
 * weight sum) in LDS -- 8 lanes and 64 slots per row up to 32 entries, a wavefront and 512 slots
 * up to 256, a workgroup of 256 threads up to GRX_LOUVAIN_BIG_ROW entries (default 4096), above
 * that a workgroup of 1024 threads with the largest table the LDS holds (GRX_LOUVAIN_LDS_SLOTS
 * lowers it; for tests) --, reads tot per occupied slot and reduces to the largest gain, then to
 * the smallest hash at that gain.  A row with more distinct neighbour communities than half the
 * table is decided on a table of two slots per entry in global memory.  label[v] is written in
 * place and tot when the class is done.  Consecutive classes of at most 1024 vertices and
 * GRX_LOUVAIN_NARROW_EDGES entries (default 16384; 0 = never) run inside one workgroup.  One
 * hand-off per sweep carries the moves, I and S; a sweep is undone from a copy of label and tot.
 * Aggregation ranks the communities by a first-occurrence pass and a scan, sorts the 64-bit keys
 * (rank[label[u]] << 32) | rank[label[v]] with their weights, sums equal keys and reads the next
 * level's offsets off the sorted keys.
 * stats may be NULL; set: iterations (the sweeps over all phases, undone and still ones included),
 * levels_recorded = min(iterations, 64), frontier_slots[t] (the moves KEPT by sweep t: 0 for an
 * undone or still sweep, so every phase ends in a 0 and the number of zeros is *h_levels),
 * vertices_reached (V - communities), edges_traversed = nnz, edges_expanded (the sum over sweeps
 * of that level graph's entry count), advance_launches, elapsed_ms and advance_kernel_ms as in
 * grx_lpa (aggregation is outside the timed batches).  The colourings' own stats are not reported.
 * The workspace is released on return and the handle keeps nothing but the symmetry verdict. */
int grx_louvain(grx_context_t ctx, grx_graph_t g, int32_t* d_community, int64_t* h_communities,
                double* h_modularity, int32_t* h_levels, const grx_options* opt, grx_stats* stats);
/* Minimum spanning FOREST of the CSR as given (the reference's mst.hxx returns one float total,
 * accumulated by float atomics, on connected graphs only, and no edges; this is not a port of it).
 * Every row entry e = (u, v, w) is an undirected candidate edge, whatever its direction; e is the
 * entry's position in the column array.  A directed CSR therefore gives the forest of its weak
 * components and needs no in-edges (attached ones are ignored).  Self loops are never chosen.
 * Repeated entries and the two stored directions of a symmetric edge are separate entries and
 * compete like any others.  Entries are strictly and totally ordered by the 64-bit key
 *     key(e) = (ordered_bits(w) << 32) | e
 * where ordered_bits maps a float's bit pattern b to ~b when its sign bit is set and to
 * b | 0x80000000 otherwise: monotone in the value, -0 below +0; the place of a NaN weight is
 * unspecified.  THE RESULT IS EXACTLY THE SET OF ENTRIES KRUSKAL ACCEPTS WHEN IT TAKES ENTRIES IN
 * ASCENDING KEY: a function of the CSR arrays alone, not of the schedule, and the same call returns
 * bit-identical outputs.  When weights tie, the chosen entries depend on the row layout (positions
 * break the ties); the total weight does not.  Every handle with entries carries values (the
 * constructors demand them), and they are read as grx_sssp reads them: as they are.
 * d_entries: device int32[V] out or NULL: the chosen entry positions in ASCENDING order, the first
 * *h_count of them valid, the rest untouched.  h_count: HOST out or NULL: the number of chosen
 * entries = V - components.  h_weight: HOST out or NULL: the float64 sum of the chosen weights, added
 * in ascending entry order by a fixed tree (no float atomics), so it is reproducible, and exact
 * whenever the float64 sum of these float32 values is.  d_component: device int32[V] out or NULL:
 * the labels grx_cc returns (the smallest vertex id of each vertex's component).  At least one of
 * the four must be non-NULL (GRX_ERR_INVALID_ARGUMENT otherwise); the call works on arrays of its own
 * either way.  n_rows != n_cols is GRX_ERR_INVALID_ARGUMENT; V == 0 is GRX_OK with count 0, weight
 * 0.0 and nothing written.  opt may be NULL; only collect_kernel_time is read, and
 * max_iterations != 0 is GRX_ERR_INVALID_ARGUMENT.
 * Method: Boruvka.  Each round, every entry whose ends lie in different components offers its key to
 * BOTH components (pre-tested 64-bit atomic min; both, because the twin stored in the other row is a
 * different candidate); every component with a key hooks under the component at the other end of
 * its entry, and when two components picked the same entry -- the only cycle a strict order allows
 * -- the smaller root id stays root and the entry is recorded once; pointer jumping flattens the
 * components; the number of hooks goes to the host, and the loop ends when at most one component
 * hooked (at most that many can still grow).  A row whose entries are all inside one component is
 * flagged and costs one byte from then on (GRX_MST_ROW_FLAGS=0 walks every row every round); rows
 * above GRX_MST_BIG_ROW entries (default 4096) are cut into segments for whole workgroups.
 * stats may be NULL; set: elapsed_ms (the whole call), advance_kernel_ms (the kernels alone, batch
 * by batch, when collect_kernel_time is set), advance_launches (kernel launches), iterations (the
 * Boruvka rounds: defined by the schedule, <= ceil(log2 V) + 1, 0 for a graph without entries),
 * vertices_reached (V - components = the count), edges_traversed = edges_expanded (row entries read
 * by the minimum-search kernels, summed over rounds).  The call runs on the caller's CSR as given,
 * builds and uses no hot-first copy, leaves nothing on the handle and releases its workspace when it
 * returns. */
int grx_mst(grx_context_t ctx, grx_graph_t g, int32_t* d_entries, int64_t* h_count, double* h_weight,
            int32_t* d_component, const grx_options* opt, grx_stats* stats);
/* Sparse matrix product C = A * B as a NEW handle (no counterpart in the reference that could be
 * ported: its algorithms/spgemm.hxx places entry (m, n) at row_offsets[m] + n, a column id used as a
 * position inside a row).  *out receives an OWNING handle of shape a.n_rows x b.n_cols that the
 * caller destroys with grx_graph_destroy and that is an ordinary handle for every other call.
 * a == b is allowed; in-edges or a hot-first copy attached to a or b are ignored; a and b are not
 * changed.  C carries no symmetry verdict (unknown), no hot-first copy and no in-edges.
 * Pattern: C has an entry (i, j) iff there is at least one pair of entries (i, k) in row i of A and
 * (k, j) in row k of B.  Each (i, j) is stored ONCE, rows are sorted by ascending column, diagonal
 * entries are kept, and an entry whose products cancel to 0.0 is still an entry: the pattern is
 * structural, a function of the two index arrays alone -- not of the values, the order of a row's
 * entries or the schedule.  Repeated entries of A or B each contribute a product, so a multigraph's
 * multiplicities multiply.
 * Values: C[i,j] is the float32 sum of A[i,k] * B[k,j] over all such pairs (each product rounded
 * once), added in an order the call does NOT promise: the sums are LDS float adds that arrive in
 * schedule order.  The value is exact, and bit-identical from call to call, whenever every partial
 * sum of those products in any order is representable in float32 -- integer weights with
 * sum |products| < 2^24 per entry, for one.  Otherwise it lies within the standard summation bound
 * of the float64 sum and may differ in the last bits between calls; a reproducible ordered sum is
 * not offered.
 * Sizes: products are counted in 64 bits.  A handle holds at most INT32_MAX entries: when nnz(C)
 * exceeds that the call returns GRX_ERR_UNSUPPORTED, the message names the count, and nothing of
 * that size has been allocated.  a.n_rows == 0, b.n_cols == 0 and operands without entries are
 * valid and give a handle with empty rows.
 * Errors: GRX_ERR_INVALID_ARGUMENT for NULL ctx, a, b or out, for a.n_cols != b.n_rows and for
 * opt->max_iterations != 0.  opt may be NULL; only collect_kernel_time is read.
 * Method: two-phase Gustavson.  One pass counts the products u(i) of every row.  The symbolic phase
 * bins the rows by min(u(i), b.n_cols) and counts each row's distinct columns in a hash table in
 * LDS (open addressing, atomicCAS on the key, load factor <= 1/2): 8 lanes per row for rows of at
 * most GRX_SPGEMM_SMALL_PRODUCTS products (default and most 32, 0 = never), a wavefront per row up
 * to 256 entries, a workgroup per row above that, its table sized from the device's LDS per
 * workgroup.  A 64-bit sum of the counts decides the refusal, a 32-bit scan gives C's row offsets.
 * The numeric phase bins the rows again by their EXACT length, accumulates a float beside each key
 * by LDS float adds, sorts the table in place (bitonic, by column) and writes the row.  Rows that
 * no table holds are walked once per TILE of columns, the tile a bitmap (and a float per column)
 * in LDS, read out in column order; there are no float atomics to global memory anywhere.
 * GRX_SPGEMM_LDS_SLOTS lowers the table capacity (and the tile with it): a test hook.
 * stats may be NULL; set: elapsed_ms (the whole call), advance_kernel_ms (the kernels alone, batch
 * by batch, when collect_kernel_time is set; 0 otherwise), advance_launches (kernel launches),
 * iterations (1), vertices_reached (rows of C with an entry), edges_traversed (nnz(C)),
 * edges_expanded (the products, sum over i of sum over k in row i of A of len(row k of B)); with
 * collect_kernel_time, levels_recorded is 3 and frontier_slots[0..2] hold the MICROSECONDS of the
 * bound, symbolic and numeric batches.  The workspace is released when the call returns. */
int grx_spgemm(grx_context_t ctx, grx_graph_t a, grx_graph_t b, grx_graph_t* out, const grx_options* opt,
               grx_stats* stats);
/* K-truss decomposition (the reference has none; nothing is ported).
 * THE TRUSSNESS OF EVERY EDGE of the simple undirected graph under a symmetric CSR.  The input may
 * be a multigraph with self loops and unsorted rows: as in grx_tc, self loops and repeated entries
 * are ignored, and the order of a row's entries does not matter.  Let m be the number of distinct
 * undirected edges that are not self loops.  The k-truss is the largest subgraph in which every
 * edge lies in at least k - 2 triangles of that subgraph, and truss(e) is the largest k >= 2 whose
 * k-truss holds e: the convention of networkx.k_truss.  An edge in no triangle has 2, every edge of
 * the complete graph on n vertices has n.  The k-truss itself is the set of entries with value >= k.
 * d_truss: device int32[nnz] out, overwritten, ONE VALUE PER CSR ENTRY in the caller's positions
 * and numbering: entry p = (u, v) carries truss({u, v}), so both directions and every repeat of an
 * edge carry the same value; a self loop carries 0.  h_max_truss: HOST out, the largest value
 * written, 0 when there is no edge but self loops (the empty graph included).  At least one of the
 * two must be non-NULL (GRX_ERR_INVALID_ARGUMENT otherwise).  The result is a function of the CSR
 * alone and bit-identical from call to call; a hot-first copy on the handle is neither built nor
 * used.
 * Undirected input only: n_rows != n_cols is GRX_ERR_INVALID_ARGUMENT; a handle with in-edges
 * attached, or a CSR that is not its own transpose (verified once when unknown), is
 * GRX_ERR_UNSUPPORTED.  n_rows == 0 or nnz == 0 is GRX_OK and launches nothing.  opt may be NULL;
 * only collect_kernel_time is read, and max_iterations != 0 is GRX_ERR_INVALID_ARGUMENT.
 * Method: the simple copy with sorted rows is built per call, and every edge gets one id, named at
 * both of its entries.  The support of an edge (its triangles) comes from listing every triangle
 * once on the degree-oriented copy, as grx_tc does, and adding one to its three edges; rows are
 * binned by length (8 lanes, a wavefront, a workgroup with the row staged in LDS, or in place when
 * it does not fit).  The peel works level by level, k = 2, 3, ...: edges with support <= k - 2
 * leave in generations, each re-intersecting its two rows and lowering the support of the two
 * other edges of every triangle it was in, never below k - 2.  A triangle that loses two or three
 * edges in one generation is charged once, by the one with the smallest id, and only to edges
 * outside that generation: the supports, the generations and so the answer do not depend on
 * scheduling.  GRX_TRUSS_NARROW_EDGES (the probes a generation
 * may have to run inside one workgroup; 0 = never) and GRX_TRUSS_LDS_IDS (lowers the staging
 * capacity) are test hooks.
 * stats may be NULL; set: elapsed_ms (the whole call), advance_kernel_ms (the kernels, batch by
 * batch, when collect_kernel_time is set; 0 otherwise), iterations (the levels k at which an edge
 * left: for m > 0 the number of DISTINCT values of the answer), advance_launches (kernel launches,
 * a library sort or scan counting as one), edges_traversed (m), edges_expanded (row entries read by
 * the support pass and the peel's intersections together); with collect_kernel_time,
 * levels_recorded is 3 and frontier_slots[0..2] hold the MICROSECONDS of building the copy and the
 * edge ids, of the support pass, and of the peel with the scatter.  The workspace (20 bytes per
 * entry for the sort, then 48 bytes per edge) is released when the call returns. */
int grx_truss(grx_context_t ctx, grx_graph_t g, int32_t* d_truss, int32_t* h_max_truss,
              const grx_options* opt, grx_stats* stats);
/* Multi-source BFS (no reference counterpart): the depths grx_bfs gives, from many sources at once.
 * h_sources: HOST int32[n_sources] in the caller's numbering; NULL = every vertex 0..V-1 (n_sources
 * must then be 0): grx_bc's convention.  Let count be the number of searches.  A vertex may appear
 * more than once: each occurrence is a search of its own, with its own row and summaries.  A non-NULL
 * list with n_sources == 0, and V == 0, are GRX_OK: no output is written and nothing is launched
 * (stats, when given, is zeroed all the same).
 * d_depths: device int32[count * V] out, overwritten, or NULL.  Row i is at elements
 * [i * V, (i + 1) * V), an index computed in 64 bits (count * V may pass 2^31), and is exactly what
 * grx_bfs(ctx, g, source_i, ...) writes: hop counts along row entries as given, 0 at the source,
 * INT32_MAX where unreached.  A directed CSR is walked along its out-entries; self loops and
 * repeated entries change nothing.  With d_depths == NULL the call computes the summaries only and
 * allocates no count * V array of its own.
 * h_reached[i] (HOST int64[count]): the vertices with a finite depth, the source included.
 * h_depth_sum[i] (HOST int64[count]): the sum of the finite depths.  h_eccentricity[i] (HOST
 * int32[count]): the largest finite depth.  Each may be NULL; at least one of the four outputs must
 * be non-NULL.  Closeness of s is (reached - 1) / depth_sum: the caller's arithmetic.
 * The result is a function of the CSR and the source list alone, bit-identical from call to call,
 * and does not depend on push, pull or how the sources fall into batches.
 * Errors, all found on the host before anything is launched: GRX_ERR_INVALID_ARGUMENT for a NULL ctx
 * or g, n_sources < 0, h_sources == NULL with n_sources != 0, a source out of range, four NULL
 * outputs, n_rows != n_cols and opt->max_iterations != 0.  With opt->direction_optimized == 1 and a
 * graph that cannot be pulled (an asymmetric CSR without in-edges; an unknown verdict is verified
 * first) the call returns what grx_bfs returns: GRX_ERR_UNSUPPORTED.
 * opt may be NULL; collect_kernel_time, direction_optimized and do_alpha (0: its default, 4) are
 * read, everything else -- the load-balance choice included -- is ignored.
 * Method: bit-parallel search ("The More the Merrier", Then et al., VLDB 2014).  The sources are
 * taken 64 at a time in list order (the last batch may be partial); bit i of a 64-bit word stands for
 * search i of the batch.  Every vertex has a word `seen` and a word in each of two frontier arrays,
 * the current level's and the next one's; a level's active list holds every vertex with a non-zero
 * frontier word once.  A PUSH level walks the active list's rows: entry (u, v) offers
 * frontier[u] & ~seen[v] & ~next[v] and, when that is not 0, ORs it into next[v] with one 64-bit
 * atomic; the lane that gets 0 back lists v.  An update pass over the new list makes the words
 * `seen`, writes depth[i * V + v] for every new bit i and counts, per bit, the vertices reached:
 * those counts are the three summaries (integer sums: order cannot matter).  With
 * direction_optimized == 1 a level whose active rows have more than nnz / do_alpha entries is PULLED
 * instead (chosen per level, no hysteresis): every vertex that still lacks a search ORs the frontier
 * words of its in-neighbours (the in-edge arrays, or its own row on a symmetric CSR) and stops
 * reading once nothing is lacking; no atomics.  The default of 4 is grx_bfs's and is not measured
 * for this kernel.  Rows above GRX_BFSM_BIG_ROW entries (default 4096; a test hook) go to whole
 * workgroups in either form.  One host hand-off per level.
 * stats may be NULL; set: elapsed_ms (the whole call), advance_kernel_ms (the kernels, batch by
 * batch, when collect_kernel_time is set), advance_launches (kernel launches), iterations (the sum
 * over batches of 1 + the largest eccentricity in the batch: defined by the answer), pull_iterations
 * (levels expanded by pulling), vertices_reached (the sum of the reached values), edges_traversed
 * (the sum, over every level of every batch, of the out-degrees of that level's active vertices:
 * the work a batch shares), edges_expanded (the row entries the expanding kernels actually read.
 * A pushed level reads every entry of its active rows, so the host adds that level's degree sum
 * and no kernel counts: the figure equals edges_traversed by construction when every level pushed.
 * A pulled level counts, on the device, the in-row entries read before its early exits, which
 * depends on the schedule and may differ between calls -- the answer cannot), levels_recorded (min(levels of the FIRST batch, 64)) and frontier_slots[L] (the vertices
 * that have depth L for at least one source of the first batch).
 * The call runs on the caller's CSR as given, builds and uses no hot-first copy, leaves nothing on
 * the handle but a symmetry verdict ensure_can_pull may have produced, and releases its workspace
 * when it returns: 32 bytes per vertex (three 64-bit words and two list slots) plus, for the lists
 * of long rows, 8 bytes per 4096 entries and 8 (12 when pulling) per GRX_BFSM_BIG_ROW entries. */
int grx_bfs_multi(grx_context_t ctx, grx_graph_t g, const int32_t* h_sources, int32_t n_sources,
                  int32_t* d_depths, int64_t* h_reached, int64_t* h_depth_sum,
                  int32_t* h_eccentricity, const grx_options* opt, grx_stats* stats);
/* Batched personalized PageRank: one rank vector per seed, 64 seeds to a wavefront.  No reference
 * counterpart: the reference's ppr.hxx is an approximate forward push with float atomics; this is the
 * power iteration of grx_pagerank restarted at one vertex, with every sum in a fixed order.
 * h_seeds: HOST int32[n_seeds] in the caller's numbering; NULL = every vertex 0..V-1 (n_seeds must
 * then be 0): the convention of grx_bc and grx_bfs_multi.  Let count be the number of seeds.  A
 * repeated seed is a column of its own.  A non-NULL list with n_seeds == 0, and V == 0, are GRX_OK:
 * nothing is written, nothing is launched, stats (when given) is zeroed.
 * Weights are read as they are, as grx_sssp and grx_pagerank read them.  W(u) is the float32 sum of
 * row u's weights, computed once per call by a fixed tree (lane l of a wavefront adds entries l,
 * l + 64, ... in order; the 64 sums meet in a butterfly).  u is DANGLING when W(u) == 0: an empty
 * row, or weights that sum to 0.  scale[u] = alpha / W(u), or 0 when dangling: grx_pagerank's
 * quantities.
 * Iteration, for seed s: p_0 = e_s and
 *   p_{t+1}[v] = sum over in-entries (u -> v, w) of (p_t[u] * scale[u]) * w
 *                + [v == s] * ((1 - alpha) + alpha * D_t),   D_t = sum of p_t[u] over dangling u.
 * Dangling mass returns to the seed (networkx.pagerank(personalization={s: 1})); each column sums to
 * 1; the mean over all V seeds is the grx_pagerank vector; alpha means what it means there.
 * Stop: column i stops after the first iteration t >= 1 with max_v |p_t[v] - p_{t-1}[v]| < tol
 * (grx_pagerank's test), and after opt->max_iterations iterations when that is non-zero.  The column
 * is FROZEN from then on: it does not change while other columns of its batch go on, so a column's
 * values do not depend on which other seeds are in the list or how they fall into batches.
 * tol <= 0 means "never by tol"; max_iterations must then be > 0.  A column that is never below tol
 * (NaN weights) ends the call with GRX_ERR_RUNTIME after 2^20 iterations.
 * d_p: device float[count * V] out, overwritten, required.  Row i is at [i * V, (i + 1) * V), an
 * index computed in 64 bits.  h_iterations (HOST int32[count], may be NULL): the iterations column i
 * ran.  h_residual (HOST float[count], may be NULL): its last max-difference.
 * Reproducibility: no float atomics.  Every sum is taken in an order fixed by the in-entry layout, V
 * and one constant, GRX_PPR_SEGMENT: the number of entries of an in-row that one lane group sums
 * (default 512, minimum 64; an environment variable read per call, a test hook).  An in-row of at
 * most that many entries is summed sequentially in row order from 0, one fused multiply-add per
 * entry; a longer one is cut into segments of that size, each summed so, and the partial sums are
 * added in segment order.  D_t is a two-stage tree over the ascending list of dangling vertices:
 * chunks of 1024 summed in list order, the chunk sums added in chunk order.  The order never depends
 * on the grid size, the CU count or arrival order: the same call returns bit-identical values, row i
 * of a batched call is bit-identical to the single-seed call, changing the hook may change last
 * bits, and whenever every term and every partial sum is representable in float32 the result is the
 * exact value.
 * Which edges: with in-edges attached (grx_graph_build_in_edges) the sum runs over those arrays and
 * their values.  Without them the handle's own rows serve as in-rows when the CSR is symmetric (an
 * unknown verdict is verified first, as for pull PageRank); an asymmetric CSR without in-edges is
 * GRX_ERR_UNSUPPORTED and the message names grx_graph_build_in_edges.
 * Errors, all found on the host before anything is launched: GRX_ERR_INVALID_ARGUMENT for a NULL ctx
 * or g, a NULL d_p with count * V > 0, n_seeds < 0, h_seeds == NULL with n_seeds != 0, a seed out of
 * range, n_rows != n_cols, alpha not in [0, 1) or NaN, a NaN tol, tol <= 0 with max_iterations == 0
 * and max_iterations < 0.
 * opt may be NULL; collect_kernel_time and max_iterations are read, everything else is ignored.
 * Method: the seeds are taken 64 at a time in list order.  State is vertex-major, p[V][L] and two
 * arrays give[V][L] = p * scale that take turns, L the smallest of 16, 32 and 64 that holds the
 * batch; lane = column, so an in-entry costs one load of (source, weight) and one contiguous
 * L * 4-byte read of give[source].  A single seed therefore idles 15 lanes of 16.  One host
 * hand-off per iteration; the rows are delivered by a transpose through LDS.
 * stats may be NULL; set: elapsed_ms (the whole call), advance_kernel_ms (the kernels, batch of
 * launches by batch, when collect_kernel_time is set), advance_launches (kernel launches),
 * iterations (the sum over batches of the batch's largest h_iterations: defined by the answer),
 * edges_traversed = edges_expanded = nnz * that sum, vertices_reached (the (seed, vertex) pairs with
 * d_p > 0, counted from the delivered values), levels_recorded (min(iterations of the FIRST batch,
 * 64)) and frontier_slots[t] (the columns of the first batch not yet frozen when its iteration
 * t + 1 begins; frontier_slots[0] is the batch's width).
 * The call builds and uses no hot-first copy, leaves nothing on the handle but a symmetry verdict
 * ensure_can_pull may have produced, and releases its workspace when it returns: per vertex 12 L
 * bytes of state (768 at L = 64), 4 of scale, 4 of the dangling list and 2 of flags; plus, per
 * GRX_PPR_SEGMENT entries of the graph, 24 bytes of lists and per segment of a long in-row 4 L bytes of partial
 * sums; plus 4 L bytes per 1024 dangling vertices. */
int grx_ppr(grx_context_t ctx, grx_graph_t g, const int32_t* h_seeds, int32_t n_seeds, float alpha,
            float tol, float* d_p, int32_t* h_iterations, float* h_residual, const grx_options* opt,
            grx_stats* stats);
/* Sparse matrix-vector product over the handle's entries, every row sum in a fixed order.  The
 * reference reaches its spmv.hxx only through headers (operators::neighborreduce, which this project
 * keeps for the header-level client); this is the same product for a C or Python caller.
 * transpose == 0: y[r] = sum over entries (r -> c, w) of row r of x[c] * w; d_x is device
 * float[n_cols], d_y device float[n_rows]; a rectangular graph is allowed.
 * transpose != 0: y[c] = sum over entries (r -> c, w) of x[r] * w, as a PULL over in-rows, never a
 * scatter: with in-edges attached (grx_graph_build_in_edges) over those arrays and their values;
 * without them over the handle's own rows when the CSR is symmetric (an unknown verdict is verified
 * first, as for grx_ppr); an asymmetric CSR without in-edges is GRX_ERR_UNSUPPORTED and the message
 * names grx_graph_build_in_edges.  The verdict is structural: a symmetric structure whose weights
 * depend on the direction needs in-edges attached.  transpose != 0 with n_rows != n_cols is
 * GRX_ERR_UNSUPPORTED.
 * d_y is overwritten in full; an empty row gives 0.0f.  Weights are read as they are.
 * Reproducibility: no float atomics.  The order of a row's sum is fixed by the row's layout and one
 * constant, GRX_SPMV_SEGMENT (default 512, minimum 64; an environment variable read per call, a test
 * hook).  A row of at most that many entries is summed by one group of 16 lanes: lane l adds entries
 * l, l + 16, ... in order, one fused multiply-add each, starting from 0, and the 16 sums meet in a
 * butterfly (lane l adds lane l ^ 8's, then l ^ 4's, l ^ 2's, l ^ 1's).  A longer row is cut into
 * segments of that size, each summed the same way by a group of its own, and a second kernel adds
 * the partial sums in segment order.  The order never depends on the grid size, the CU count or
 * arrival order: two calls return the same bits, changing the hook may change last bits, and whenever
 * every term and every partial sum is representable in float32 the result is the exact value.
 * V == 0 or an empty output (no rows to write) is GRX_OK: nothing is launched, stats (when given) is
 * zeroed.  GRX_ERR_INVALID_ARGUMENT, found on the host before anything is launched: a NULL ctx or g,
 * a NULL d_x or d_y whose length is above 0, and [d_x, d_x + len) overlapping [d_y, d_y + len).
 * opt may be NULL; only collect_kernel_time is read.  stats may be NULL; set: elapsed_ms,
 * advance_kernel_ms (with collect_kernel_time), advance_launches (kernel launches), iterations = 1,
 * edges_traversed = edges_expanded = nnz; everything else 0.
 * The call leaves nothing on the handle but a symmetry verdict and releases its workspace when it
 * returns: none for a graph of at most GRX_SPMV_SEGMENT entries, otherwise 32 bytes per
 * GRX_SPMV_SEGMENT entries of the graph (the lists of long rows and their segments, and one partial
 * sum per segment). */
int grx_spmv(grx_context_t ctx, grx_graph_t g, int32_t transpose, const float* d_x, float* d_y,
             const grx_options* opt, grx_stats* stats);
/* Sparse-dense product Y = A X over the handle's entries for a dense feature matrix, every output
 * element summed in a written order: the aggregation step of a message-passing layer, and with
 * transpose its backward pass.  An addition: the reference has an experiment of this
 * (examples/experiments/spmm.cu) and no algorithm header.
 * F = n_features.  Both matrices are row-major float32: row i of X starts at d_x + i * ldx and row i
 * of Y at d_y + i * ldy, with ldx, ldy >= F in elements.
 * transpose == 0: Y[r, f] = sum over entries (r -> c, w) of row r of X[c, f] * w; X has n_cols rows
 * and Y has n_rows rows; a rectangular graph is allowed.
 * transpose != 0: Y[c, f] = sum over entries (r -> c, w) of X[r, f] * w, as a PULL over in-rows,
 * never a scatter, under grx_spmv's rule: with in-edges attached (grx_graph_build_in_edges) over
 * those arrays and their values; without them over the handle's own rows when the CSR is symmetric
 * (an unknown verdict is verified first); an asymmetric CSR without in-edges is GRX_ERR_UNSUPPORTED
 * and the message names grx_graph_build_in_edges.  transpose != 0 with n_rows != n_cols is
 * GRX_ERR_UNSUPPORTED.
 * What is written: columns [0, F) of every row of Y are overwritten, an empty row gives 0.0f in all
 * of them.  Columns [F, ldy) of Y are never written and never read, and neither are [F, ldx) of X.
 * Weights and features are read as they are: a zero weight times an infinite feature is NaN and is
 * delivered as such; no entry is skipped for its weight.
 * Summation order (the reproducibility contract): no float atomics.  With S = GRX_SPMM_SEGMENT
 * (default 512, minimum 64; an environment variable read per call, a test hook) and a fixed output
 * element, the row's entries are cut into segments of S consecutive entries, the last one may be
 * shorter.  A segment's partial sum starts from 0.0f and takes its entries IN ROW ORDER, one fused
 * multiply-add each: acc = fma(X[c, f], w, acc).  A row of at most S entries delivers that sum; a
 * longer row delivers ((p0 + p1) + p2) + ... in segment order with plain float32 adds.  The order is
 * a function of the row's layout and S alone: it does not depend on F, ldx, ldy, the pointers'
 * alignment, the grid, the CU count or arrival order.  So two calls return the same bits; column f
 * of an F-wide call is bit-identical to the F = 1 call on that column; and where every term and
 * every partial sum is representable in float32 the result is the exact value.  The order is NOT
 * grx_spmv's (16 interleaved lanes and a butterfly): the two calls agree bit for bit only where both
 * are exact.
 * F == 0, or an output without rows, is GRX_OK: nothing is launched, stats (when given) is zeroed.
 * GRX_ERR_INVALID_ARGUMENT, found on the host before anything is launched, each message naming
 * grx_spmm: a NULL ctx or g; n_features < 0; ldx < F or ldy < F; a NULL d_x or d_y whose matrix has
 * elements; the byte range of X overlapping that of Y (the message says "overlap"), a range being
 * first element to last element, (rows - 1) * ld + F elements long -- two interleaved views of one
 * buffer overlap in this sense although they share no element.
 * opt may be NULL; only collect_kernel_time is read.  stats may be NULL; set: elapsed_ms,
 * advance_kernel_ms (with collect_kernel_time), advance_launches (kernel launches: 1 for a graph of
 * at most S entries, otherwise 4 -- the plan, the short rows, the segments, their sums),
 * iterations = 1, edges_traversed = edges_expanded = nnz; everything else 0.
 * The call runs on the caller's CSR and numbering as given, builds and uses no hot-first copy, leaves
 * nothing on the handle but a symmetry verdict and releases its workspace when it returns: none for a
 * graph of at most S entries, otherwise 32 bytes per S entries of the graph (the lists of long rows
 * and their segments) and 4 F bytes per segment the lists have room for (the partial sums).
 * Every element offset into X and Y (row * ld + f) is computed in 64 bits: n_rows * ldy may exceed
 * 2^31.  Accesses are 16 bytes wide where the base pointer is 16-byte aligned and ld % 4 == 0, and
 * narrower otherwise; the result does not depend on it. */
int grx_spmm(grx_context_t ctx, grx_graph_t g, int32_t transpose, int32_t n_features,
             const float* d_x, int64_t ldx, float* d_y, int64_t ldy,
             const grx_options* opt, grx_stats* stats);
/* grx_spmm with the caller's per-entry values: Y = A(w) X, where A(w) has the handle's structure and
 * d_values[e] (device float[nnz], in the order of the CSR's entries, the order of the column array)
 * in place of the handle's value of entry e.  The handle's own values are not read.  With
 * grx_sddmm, its derivative, this is a message-passing layer whose edge coefficients are computed
 * per step (attention, gates, learned edge weights) and their backward pass.  An addition: the
 * reference has no counterpart.
 * grx_spmm's whole contract holds with that one substitution -- matrices, leading dimensions, what
 * is written, values read as they are, the summation order with its hook GRX_SPMM_SEGMENT, stats,
 * workspace -- and the result is bit for bit what grx_spmm returns on a handle built from the same
 * structure with those values.
 * transpose != 0: Y[c, f] = sum over entries e = (r -> c) of X[r, f] * d_values[e], a pull over the
 * attached in-rows; the call first gathers d_values into in-entry order through the entry ids that
 * grx_graph_build_in_edges keeps (one more launch, 4 nnz bytes of workspace released on return).
 * Without in-edges attached the transposed call is GRX_ERR_UNSUPPORTED and the message names
 * grx_graph_build_in_edges -- on a handle known to be symmetric too: its rows are its in-rows
 * structurally, but the value of the mirror entry (c -> r) sits elsewhere in d_values, and only the
 * entry ids say where.  transpose != 0 with n_rows != n_cols is GRX_ERR_UNSUPPORTED.
 * GRX_ERR_INVALID_ARGUMENT, found on the host before anything is launched, each message naming
 * grx_spmm_values: grx_spmm's list; a NULL d_values with nnz > 0; the byte range of d_values
 * overlapping that of Y.  d_values may overlap X. */
int grx_spmm_values(grx_context_t ctx, grx_graph_t g, const float* d_values, int32_t transpose,
                    int32_t n_features, const float* d_x, int64_t ldx, float* d_y, int64_t ldy,
                    const grx_options* opt, grx_stats* stats);
/* Sampled dense-dense product: one dot product per entry of the handle's CSR,
 *   d_out[e] = sum over f < F of U[row(e), f] * V[col(e), f],
 * at the entry's position e in the column array: the edge scores of an attention or gating layer,
 * and the gradient of grx_spmm_values with respect to its values (U = the incoming gradient, V = X).
 * An addition: the reference has no counterpart.
 * F = n_features.  U and V are row-major float32: row i of U starts at d_u + i * ldu and U has n_rows
 * rows; row j of V starts at d_v + j * ldv and V has n_cols rows; ldu, ldv >= F in elements.  A
 * rectangular graph is allowed.  U and V may overlap or be the same matrix.  d_out has exactly nnz
 * elements, all overwritten; nothing before or after them is touched.  Columns [F, ld) of U and V are
 * never read.  The handle's values are not read and in-edges are not needed; duplicate entries of a
 * row each get their own, identical result.  Features are read as they are (0 * inf is NaN).
 * Summation order (the reproducibility contract): no float atomics.  The features are cut into tiles
 * of 256 consecutive features, the last one may be shorter.  Within a tile of n features let L be
 * the smallest power of two >= ceil(n / 4).  Lane l of L owns features 4 l .. 4 l + 3 of the tile; its
 * partial starts from 0.0f and takes those of its features that lie below F in ascending order, one
 * fused multiply-add each: p = fma(U[r, f], V[c, f], p) (a lane without features keeps 0.0f).  The L
 * partials are combined by the butterfly p[l] = p[l] + p[l ^ d] for d = L / 2, L / 4, ..., 1 with
 * plain float32 adds; float32 addition is commutative bit for bit, so every lane ends with the same
 * value, the tile's sum.  Tile sums are added in ascending tile order, ((t0 + t1) + t2) + ...
 * The order is a function of F alone: it does not depend on the row, its length or layout, on
 * GRX_SDDMM_SEGMENT (default 512, minimum 64; an environment variable read per call, a test hook:
 * the entries of a longer row are handed to several lane groups), on ldu, ldv, the pointers'
 * alignment, the grid, the CU count or arrival order.  So two calls return the same bits, an entry's
 * result is that of a one-row graph holding only its row, and where every term and every partial sum
 * is representable in float32 the result is the exact value.
 * F == 0: every d_out[e] = 0.0f.  nnz == 0 is GRX_OK: nothing is launched, stats (when given) is
 * zeroed.
 * GRX_ERR_INVALID_ARGUMENT, found on the host before anything is launched, each message naming
 * grx_sddmm: a NULL ctx or g; n_features < 0; ldu < F or ldv < F; a NULL d_u, d_v or d_out whose
 * array has elements; the byte range of d_out overlapping that of U or of V (the message says
 * "overlap"), a range being first element to last element as for grx_spmm.
 * opt may be NULL; only collect_kernel_time is read.  stats may be NULL; set: elapsed_ms,
 * advance_kernel_ms (with collect_kernel_time), advance_launches (kernel launches: 1 for a graph of
 * at most GRX_SDDMM_SEGMENT entries, otherwise 3 -- the plan, the short rows, the long rows' items;
 * 0 for F == 0, which is a memset), iterations = 1, edges_traversed = edges_expanded = nnz;
 * everything else 0.
 * The call runs on the caller's CSR and numbering as given, builds and uses no hot-first copy, leaves
 * nothing on the handle and releases its workspace when it returns: none for a graph of at most
 * GRX_SDDMM_SEGMENT entries, otherwise 32 bytes per GRX_SDDMM_SEGMENT entries of the graph (the lists
 * of long rows and their items).  Every element offset into U and V (row * ld + f) is computed in 64
 * bits.  Accesses are 16 bytes wide where both base pointers are 16-byte aligned and ldu % 4 == 0 and
 * ldv % 4 == 0, and narrower otherwise; the result does not depend on it. */
int grx_sddmm(grx_context_t ctx, grx_graph_t g, int32_t n_features,
              const float* d_u, int64_t ldu, const float* d_v, int64_t ldv,
              float* d_out, const grx_options* opt, grx_stats* stats);
/* Edge softmax: per-entry scores normalised over the entries that share a row, or a column,
 *   d_out[e] = exp(s[e] - m) / sum over the group's entries e' of exp(s[e'] - m),  m = max s[e'],
 * the step between grx_sddmm's scores and grx_spmm_values's coefficients in an attention layer (GAT,
 * graph transformers; DGL's edge_softmax, PyG's softmax(src, index)).  An addition: the reference has
 * no counterpart.
 * d_scores and d_out are device float[nnz] in the order of the CSR's column array -- grx_sddmm's
 * output, grx_spmm_values's input -- and d_out is overwritten in full; nothing before or after its
 * nnz elements is touched.  The handle's values and column ids are not read.  A group is the set of
 * entries of one row (by_column == 0) or of one column (by_column != 0), a column's entries taken in
 * ascending position in the CSR: the order of the in-rows that grx_graph_build_in_edges builds, which
 * sorts entry ids stably by destination.  by_column reaches an entry through those entry ids where
 * it walks; nothing is gathered or scattered in a pass of its own.
 * Arithmetic (the reproducibility contract): no float atomics.  Per group with entries e_0 .. e_{n-1}
 * in group order: m is the largest score (a maximum does not depend on order); p[e] = expf(s[e] - m),
 * one rounded subtraction and the precise exponential; S is the sum of p in grx_spmv's row order: the
 * group is cut into segments of GRX_SOFTMAX_SEGMENT consecutive entries (default 512, minimum 64; an
 * environment variable read per call, a test hook), within a segment lane l of 16 adds entries l,
 * l + 16, ... in order starting from 0.0f, the 16 lane sums meet in the butterfly x[l] = x[l] + x[l ^ d]
 * for d = 8, 4, 2, 1, and the segment sums are added in segment order, ((0.0f + S0) + S1) + ... for a
 * group of more than one segment; d_out[e] = p[e] / S, a correctly rounded division.
 * Edge cases: an empty group writes nothing.  A group that holds a NaN or a +inf score gets NaN in
 * every entry, as torch.softmax gives -- also when its other scores are all -inf: the maximum
 * propagates NaN.  A group whose scores are all -inf (fully masked) gets 0.0f in every entry, no NaN.
 * -inf beside finite scores gives an exact 0 for that entry.  No other group is affected by any of these.
 * Consequences: the same call returns the same bits.  A group's results depend on that group's
 * values, its length and the segment alone -- not on the grid, the CU count, the other groups or where
 * the group sits: they are those of a one-group graph.  Equal scores give exactly 1 / n for n up to
 * 2^24; adding a constant that leaves every s[e] - m unchanged leaves every bit unchanged.  by_column
 * on a symmetric CSR whose mirror entries carry equal scores gives the row result at the mirror
 * positions.
 * nnz == 0 is GRX_OK: nothing is launched, stats (when given) is zeroed.
 * GRX_ERR_INVALID_ARGUMENT, found on the host before anything is launched, each message naming the
 * call: a NULL ctx or g; a NULL d_scores or d_out while nnz > 0; the byte range of d_out overlapping
 * that of d_scores (the message says "overlap").  GRX_ERR_UNSUPPORTED: by_column without in-edges
 * attached, on a handle known to be symmetric too (the message names grx_graph_build_in_edges): only
 * the entry ids say where a column's entries sit; by_column with n_rows != n_cols.
 * opt may be NULL; only collect_kernel_time is read.  stats may be NULL; set: elapsed_ms,
 * advance_kernel_ms (with collect_kernel_time), advance_launches (kernel launches: 1 for a graph of
 * at most GRX_SOFTMAX_SEGMENT entries, otherwise 6 -- the plan, the short groups, and for the long
 * ones their items' maxima, their items' sums, the totals, the quotients), iterations = 1,
 * edges_traversed = edges_expanded = nnz; everything else 0.
 * The call leaves nothing on the handle and releases its workspace when it returns: none for a graph
 * of at most GRX_SOFTMAX_SEGMENT entries, otherwise 48 bytes per GRX_SOFTMAX_SEGMENT entries of the
 * graph (the lists of long groups and their items; a partial sum, a total and a maximum per item). */
int grx_edge_softmax(grx_context_t ctx, grx_graph_t g, int32_t by_column, const float* d_scores,
                     float* d_out, const grx_options* opt, grx_stats* stats);
/* The derivative of grx_edge_softmax: with a = d_probabilities (its output) and t = d_grad (the
 * gradient with respect to that output), the gradient with respect to the scores,
 *   d_out[e] = a[e] * (t[e] - D),  D = sum over the group's entries e' of a[e'] * t[e'].
 * Arrays, groups, by_column, the segment hook, refusals (a NULL d_probabilities, d_grad or d_out while
 * nnz > 0; d_out overlapping either input; the inputs may overlap each other), nnz == 0 and stats are
 * grx_edge_softmax's; advance_launches is 1, or 5 for a graph of more than GRX_SOFTMAX_SEGMENT
 * entries (the plan, the short groups, the items' sums, the totals, the results).
 * Arithmetic: D is summed in the segment, lane and butterfly order of S above, one fused
 * multiply-add per entry, acc = fma(a[e], t[e], acc) from 0.0f; d_out[e] = a[e] * (t[e] - D) with one
 * rounded subtraction and one rounded multiplication, not fused.  a need not be a softmax result.
 * The same call returns the same bits, and a group's results are those of a one-group graph. */
int grx_edge_softmax_backward(grx_context_t ctx, grx_graph_t g, int32_t by_column,
                              const float* d_probabilities, const float* d_grad, float* d_out,
                              const grx_options* opt, grx_stats* stats);
/* HITS: hub and authority scores by power iteration, two pull products per iteration.  It REPLACES
 * the reference's hits.hxx rather than wrapping it: that client does one float atomic per edge in each
 * direction, normalises by an L2 norm and stops on bit-equality of two vectors, so it neither repeats
 * itself nor has a stable answer.  Here, with weights read as they are, h_0 = 1 at
 * every vertex and for t = 1, 2, ...
 *   y[v] = sum over in-entries  (u -> v, w) of h_{t-1}[u] * w;  a_t = y / max_v |y[v]|
 *   z[u] = sum over out-entries (u -> v, w) of a_t[v] * w;      h_t = z / max_u |z[u]|
 *   residual_t = max_v |h_t[v] - h_{t-1}[v]|
 * where a vector whose largest magnitude is 0 stays all 0.  The division is carried out as a
 * multiplication by the rounded reciprocal of the maximum, the same arithmetic wherever a value is
 * used or delivered: the largest entry of a delivered vector is 1 to within that one rounding, and
 * exactly 1 when the maximum is a power of two.  Rescaling to sum 1 (networkx) or to L2 norm 1 (the
 * reference) is the caller's arithmetic.
 * Stop: after the first t >= 1 with residual_t < tol (grx_pagerank's and grx_ppr's test), and after
 * opt->max_iterations iterations when that is non-zero.  tol <= 0 means "never by tol";
 * max_iterations must then be > 0.  A run that is never below tol (NaN weights) ends with
 * GRX_ERR_RUNTIME after 2^20 iterations.
 * d_hub, d_authority: device float[V] out, overwritten; either may be NULL, not both when V > 0, and
 * leaving one out does not change a bit of the other.  h_iterations (HOST int32, may be NULL): t.
 * h_residual (HOST float, may be NULL): the last residual_t.
 * Reproducibility: a maximum and a largest difference are the same bits in any reduction order, so
 * the iteration is order-free except its row sums, and those follow the rule of grx_spmv with the
 * same constant GRX_SPMV_SEGMENT: no float atomics, the same call returns the same bits, and where
 * every term and every partial sum is representable in float32 the result is the exact value.
 * Which edges (grx_ppr's rule): with in-edges attached the in-product runs over those arrays and
 * their values and the out-product over the rows.  Without them the rows serve both products when
 * the CSR is symmetric (an unknown verdict is verified first); an asymmetric CSR without in-edges is
 * GRX_ERR_UNSUPPORTED and the message names grx_graph_build_in_edges.  The verdict is structural: a
 * caller whose symmetric structure carries direction-dependent weights attaches in-edges.
 * Errors, all found on the host before anything is launched, GRX_ERR_INVALID_ARGUMENT: a NULL ctx or
 * g, both outputs NULL with V > 0, n_rows != n_cols, a NaN tol, tol <= 0 with max_iterations == 0,
 * max_iterations < 0.  V == 0 is GRX_OK: nothing is written, nothing is launched.  A graph without
 * entries follows the definition: a_1 = h_1 = 0, residual_1 = 1, residual_2 = 0.
 * opt may be NULL; collect_kernel_time and max_iterations are read, everything else is ignored.
 * Method: the products y and z are kept unnormalised and the scale is applied where the next product
 * gathers a value, so normalising costs no pass of its own; the residual is one pass over two
 * vectors, left out in the iterations whose residual nobody reads (tol <= 0, all but the last).  With
 * tol > 0 there is one host hand-off per iteration; with tol <= 0 the whole run is enqueued without
 * a host wait and the figures are read once at the end.
 * stats may be NULL; set: elapsed_ms, advance_kernel_ms (with collect_kernel_time),
 * advance_launches (kernel launches), iterations = t, edges_traversed = edges_expanded =
 * 2 * nnz * t, vertices_reached (the vertices with hub > 0 or authority > 0, counted from the
 * delivered values); everything else 0.
 * The call builds and uses no hot-first copy, leaves nothing on the handle but a symmetry verdict
 * ensure_can_pull may have produced, and releases its workspace when it returns: 12 bytes per vertex
 * (y and two z) and, for a graph of more than GRX_SPMV_SEGMENT entries, 32 bytes per
 * GRX_SPMV_SEGMENT entries of the graph (the lists of long rows and their segments, 8 bytes per
 * long row and 12 per segment at most), twice with in-edges attached. */
int grx_hits(grx_context_t ctx, grx_graph_t g, float tol, float* d_hub, float* d_authority,
             int32_t* h_iterations, float* h_residual, const grx_options* opt, grx_stats* stats);
/* Shortest-path trees: the predecessors that finished labels imply, a count of the entries that
 * contradict the labels, and (SSSP) hop counts along the tree.  The reference left predecessors as a
 * "@todo" (bfs.hxx:28) and grx_bfs / grx_sssp ignore the argument; these two calls derive the tree in
 * one pass over the entries from what those calls delivered.  The labels (d_depths: device int32[V],
 * INT32_MAX = unreached; d_distances: device float[V], FLT_MAX = unreached) are in the caller's
 * numbering and are plain input: any array is accepted, and the results are a function of the CSR
 * arrays, the labels and the source alone.
 * For every row entry (u, v, w) whose label[u] is not the unreached value:
 *   BFS   the entry QUALIFIES when depth[u] + 1 == depth[v] and VIOLATES when depth[u] + 1 < depth[v]
 *         (in 64-bit integers);
 *   SSSP  with c = dist[u] + w as ONE float32 add, it qualifies when c == dist[v] and dist[u] < dist[v],
 *         and violates when c < dist[v].  A NaN makes every comparison false: it qualifies nothing and
 *         violates nothing.
 * The add is the one every relaxation of grx_sssp performs, pushed or pulled, so at its fixed point
 * every reached vertex but the source has a qualifying entry bit for bit.
 * d_predecessors (device int32[V] out): for a reached v != source the SMALLEST u with a qualifying
 * entry into v; every qualifying entry lowers the label strictly, so chains of predecessors never
 * cycle, whatever the input.  d_predecessors[source] = source (the Graph500 convention); -1 for an
 * unreached v; -2 for an ORPHAN, a reached vertex other than the source without a qualifying entry.
 * On the labels of a finished search an orphan exists only where a zero weight, or a weight absorbed
 * by rounding, leaves dist[v] == dist[u]; on integer weights >= 1 with distances below 2^24, and on
 * any BFS result, there is none.
 * h_orphans (HOST int64): the orphans.  h_violations (HOST int64): the violating entries, 0 exactly
 * when the labels are a fixed point of relaxation; a search cut off by max_iterations shows here.
 * d_hops (SSSP only, device int32[V] out, may be NULL): the predecessor steps from v to the source, 0
 * at the source, -1 for a vertex that is unreached, an orphan, or whose chain ends in an orphan.  (For
 * BFS it would equal the depth.)
 * d_predecessors may be NULL when another output is asked for (the call then works on an array of its
 * own); every output NULL is GRX_ERR_INVALID_ARGUMENT.  So are, all found before anything is
 * launched: a NULL ctx, g or labels; n_rows != n_cols; opt->max_iterations != 0; source out of range;
 * label[source] != 0 (read by a 4-byte copy on the context's stream).  V == 0 is GRX_OK with both
 * counts 0 and nothing written.  opt may be NULL; only collect_kernel_time is read.
 * Which entries: the call runs on the caller's CSR as given.  It neither builds nor uses a hot-first
 * copy, starts no symmetry verification, leaves nothing on the handle and releases its workspace on
 * return (at most 4 bytes per vertex without d_predecessors, 16 per vertex with d_hops, 24 bytes per
 * GRX_TREE_SEGMENT entries).  Two forms of the pass give the same outputs.  PULL walks in-rows with a
 * group of 16 lanes per vertex and no atomics on rows of at most GRX_TREE_SEGMENT entries (default
 * 512, minimum 64; an environment variable read per call, a test hook); it runs when in-edges are
 * attached (their values are the entries' weights), or the handle's symmetry verdict is ALREADY
 * "symmetric" (for SSSP: and its builder vouched for equal weights in both directions, as grx_sssp
 * asks before it pulls).  PUSH walks out-rows and lowers d_predecessors[v] by a 32-bit atomicMin; it
 * runs in every other case, and whenever GRX_TREE_PULL=0.  Only integer minima, integer sums and
 * plain stores are used: the same call returns bit-identical outputs, in either form.
 * d_hops is pointer doubling on 8-byte {ancestor, steps} pairs in two buffers that take turns, four
 * rounds enqueued per host hand-off (a round past the last changing one copies its input); more than
 * 32 rounds is GRX_ERR_RUNTIME (chains shorter than 2^31 need fewer).
 * stats may be NULL; set: elapsed_ms, advance_kernel_ms (with collect_kernel_time), advance_launches
 * (kernel launches), vertices_reached (the labels that are not the unreached value), edges_traversed
 * = edges_expanded = nnz, pull_iterations (1 when the pull form ran, else 0), iterations (0 without
 * d_hops, else ceil(log2(L)), L the largest number of predecessor steps from any vertex to the end
 * of its chain, the source or an orphan; 0 for L <= 1); everything else 0. */
int grx_bfs_predecessors(grx_context_t ctx, grx_graph_t g, int32_t source, const int32_t* d_depths,
                         int32_t* d_predecessors, int64_t* h_orphans, int64_t* h_violations,
                         const grx_options* opt, grx_stats* stats);
int grx_sssp_predecessors(grx_context_t ctx, grx_graph_t g, int32_t source, const float* d_distances,
                          int32_t* d_predecessors, int32_t* d_hops, int64_t* h_orphans,
                          int64_t* h_violations, const grx_options* opt, grx_stats* stats);
/* Random walks: first-order uniform and weighted walks and node2vec (second-order, by rejection),
 * the corpus of DeepWalk / node2vec and of random-walk samplers.  No reference counterpart.  Every
 * draw comes from a counter-based generator, so the answer is a function of the CSR and the arguments
 * alone: walk i is the same bits in every call, and depends neither on the schedule, nor on how walks
 * are grouped into launches, nor on which other walks are in the list.
 * h_starts: HOST int32[n_starts]; NULL = every vertex 0..V-1 (n_starts must then be 0): the convention
 * of grx_bc, grx_bfs_multi and grx_ppr.  Let count be the number of walks; a vertex named twice is two
 * walks with different draws.  A non-NULL list with n_starts == 0, and V == 0, are GRX_OK: nothing is
 * written, nothing is launched, stats (when given) is zeroed.
 * d_walks: device int32[count * (length + 1)] out, row-major, indexed in 64 bits, required.  Row i is
 * start_i, v_1, ..., v_length; a walk that meets a DEAD END stops there and its remaining slots are
 * -1.  A dead end is an empty row and, when `weighted`, a row whose total W (below) is not > 0.
 * length == 0 writes the starts only.  A directed CSR is walked along its out-entries; attached
 * in-edges are ignored.  A repeated entry counts each time it appears; a self loop is a step like
 * any other.
 * Draws, with mix64 the splitmix64 finaliser of x + 0x9E3779B97F4A7C15 (grx_graph_rmat's):
 *   r(i, t, j) = mix64(mix64(seed ^ mix64(i)) + ((uint64)t << 32) + j)   mod 2^64,
 * i the 64-bit index of the walk in the list, t = 1..length the step, j the draw inside the step, and
 * u24(r) = (float)(r >> 40) * 2^-24, exact and in [0, 1).
 * Candidate of row v (d entries, in row order) from a draw r:
 *   weighted == 0: entry k = ((r >> 32) * d) >> 32 in 64-bit integers.  Entries are not exactly
 *     equally likely: the bias is at most d / 2^32 per entry.
 *   weighted != 0: probability proportional to the entry's float value, through a prefix array c whose
 *     order is part of the definition.  The row is cut into blocks of 64 entries in row order; inside
 *     block b, l_k is the sequential float32 sum of the block's weights up to k; the block bases are
 *     B_0 = 0, B_{b+1} = fl(B_b + l_last(b)); c_k = fl(B_b + l_k), non-decreasing for non-negative
 *     weights; W = c_{d-1}; x = fl(u24(r) * W).  The candidate is the smallest k with c_k > x and, when
 *     there is none (the product rounded up to W), the smallest k with c_k == W.  An entry of weight 0
 *     is never chosen.  With negative or NaN weights the result is unspecified, but the search never
 *     leaves the row.
 * Step t of walk i at v, having come from prev (none at t == 1): attempts a = 0, 1, ...; the candidate
 * x of attempt a comes from r(i, t, 2a); it is accepted at once when t == 1 or ratio == 1, otherwise
 * iff u24(r(i, t, 2a + 1)) < ratio, where ratio is `ret` if x == prev, `adj` if the entry prev -> x
 * exists (whatever the order of row prev) and `far` otherwise.  The three are computed once, in
 * float32: ip = 1/p, iq = 1/q, m = max(ip, 1, iq), ret = ip / m, adj = 1 / m, far = iq / m: node2vec
 * by rejection.  With p == q == 1 every ratio is 1 and the walk is the first-order walk, bit for bit.
 * After GRX_WALK_MAX_ATTEMPTS rejected attempts the last candidate is taken (default and maximum
 * 1024, minimum 1; an environment variable read per call, a test hook).  The cap makes the loop
 * finite and is a bias: with p, q in [0.125, 8] the smallest ratio is 1/64, so a step reaches the cap
 * with probability below (63/64)^1024, about 1e-7, and then takes a candidate it might have rejected.
 * Errors, all found on the host before anything is launched: GRX_ERR_INVALID_ARGUMENT for a NULL ctx
 * or g, n_starts < 0, h_starts == NULL with n_starts != 0, a start out of range, length < 0,
 * n_rows != n_cols, p or q NaN or outside [0.125, 8], a NULL d_walks with count > 0 and V > 0, and
 * opt->max_iterations != 0.  opt may be NULL; only collect_kernel_time is read.
 * Method: one lane per walk, one launch.  A weighted call first builds c (4 bytes per entry, plus 4
 * per block of 64 and 4 per vertex while it is built) and selects by binary search in it; a call with
 * p != 1 or q != 1 and length > 1 first builds a copy of the columns with every row sorted (4 bytes
 * per entry; 16 more and the sort's workspace while it is built), in which it looks prev -> x up.
 * Both are built per call; no hot-first copy is built or used, nothing is left on the handle, and the
 * workspace is released on return.
 * stats may be NULL; set: elapsed_ms (the whole call), advance_kernel_ms (its kernels, when
 * collect_kernel_time is set), advance_launches (this library's kernels: the walker, 3 more for c, 2
 * more for the sorted rows), iterations (the largest number of steps any walk took),
 * vertices_reached (walks that took all `length` steps), edges_traversed (steps taken: the
 * non-negative entries of d_walks minus count), edges_expanded (candidates drawn; equal to
 * edges_traversed when p == q == 1), levels_recorded (min(iterations, 64)) and frontier_slots[t - 1]
 * (walks that took step t). */
int grx_random_walk(grx_context_t ctx, grx_graph_t g, const int32_t* h_starts, int32_t n_starts,
                    int32_t length, uint64_t seed, int32_t weighted, float p, float q,
                    int32_t* d_walks, const grx_options* opt, grx_stats* stats);
/* Neighbour sampling: multi-hop fan-out sampling WITHOUT replacement, the mini-batch sampler of
 * GraphSAGE-style training (PyG's NeighborLoader, DGL's sample_neighbors, cuGraph's
 * uniform_neighbor_sample).  No reference counterpart.  Every draw comes from grx_random_walk's
 * counter-based generator, so the answer is a function of the CSR and the arguments alone: the same
 * bits in every call, whatever the schedule and the lane-group widths.
 * Seeds.  h_seeds: HOST int32[n_seeds]; NULL = every vertex 0..V-1 (n_seeds must then be 0): the
 * convention of grx_bc, grx_bfs_multi, grx_ppr and grx_random_walk.  Repeats are dropped and the first
 * occurrence is kept: level 0 of the node list is the distinct seeds in list order.  A non-NULL list
 * with n_seeds == 0, and V == 0, are GRX_OK: nothing is launched, device outputs are untouched,
 * offsets (when given) are all 0, stats (when given) is zeroed.
 * Fan-outs.  h_fanouts: HOST int32[n_hops], 1 <= n_hops <= 64.  k_h in [1, 1024]: at most k_h entries
 * of each expanded row; k_h == -1: every entry; k_h == 0, k_h < -1 and k_h > 1024 are errors.
 * Levels.  Node level 0 is the seeds.  Hop h = 1..n_hops expands exactly the vertices of level h - 1,
 * in node-list order: a vertex is expanded at most once per call, in the hop after it was first
 * reached (PyG's convention).  Level h is the set of vertices named by hop h's sampled entries that
 * are in no earlier level, in ascending vertex id.  A vertex's LOCAL id is its index in the node
 * list.  When a level is empty every later hop samples nothing.
 * Sample of row v in hop h.  Let d be the row's length, its positions ap[v] .. ap[v] + d - 1 as given,
 * and k = k_h.
 *   All: k == -1 or d <= k.  Every entry is taken; no draws are made.
 *   Otherwise the candidates are x_a = walk_pick_uniform(r(v, h, a), d) = ((r >> 32) * d) >> 32 for
 *   a = 0, 1, ..., with r(v, h, a) = walk_draw(walk_stream(seed, v), h, a): r(i, t, j) of
 *   grx_random_walk with i = the vertex id, t = the hop (1-based) and j = the attempt.  Let m = k when
 *   2k <= d (INCLUDE), else m = d - k (EXCLUDE), so m <= d / 2 always.  S is the first m distinct
 *   values of the sequence, and A the number of candidates drawn until S is complete: the smallest A
 *   for which x_0 .. x_{A-1} hold m distinct values.  Include takes the positions in S; exclude takes
 *   every position of the row not in S.  The chosen entries are emitted in ascending position.
 *   Every k-subset of the row is equally likely, up to walk_pick_uniform's bias of d / 2^32 per
 *   entry.  The draws are keyed by the vertex, not by its place in the frontier: the sample of row v
 *   in hop h under `seed` is the same whichever other seeds are in the list.  A caller varies `seed`
 *   per batch.
 *   The loop is bounded at 64 m + 1024 attempts; reaching the bound sets a device flag and the call
 *   returns GRX_ERR_RUNTIME.  This cannot happen unless the kernels are wrong: while fewer than
 *   m <= d / 2 positions are held, an attempt names a new one with probability at least
 *   1/2 - d / 2^33 > 1/4, so the new positions among n = 64 m + 1024 attempts dominate a binomial
 *   (n, 1/4) count X, and by Hoeffding P(X < m) <= exp(-2 (n/4 - m)^2 / n) with
 *   n/4 - m = 15 m + 256 > 15 (m + 16) and n = 64 (m + 16): below exp(-7 (m + 16)) <= e^-119 < 2^-171
 *   per row.
 * Graph conventions.  A repeated entry is an entry of its own: a sample may hold both copies.  A self
 * loop is an entry like any other (dst == src, no new vertex).  An empty row contributes nothing.  A
 * directed CSR is sampled along its out-entries; attached in-edges and a hot-first copy are ignored
 * and none is built: a host that wants in-neighbours passes the transposed graph.  Float values are
 * ignored.
 * Outputs.  Each may be NULL, but not all six; with device outputs NULL the call works on arrays of
 * its own, so a count-only call is possible.
 *   d_nodes: device int32[node_capacity]: vertex ids in the caller's numbering, in local-id order.
 *   h_node_offsets: HOST int64[n_hops + 2]: level L is [off[L], off[L + 1]).
 *   d_src, d_dst: device int32[edge_capacity]: the LOCAL ids of the expanded vertex and of the
 *     sampled neighbour.
 *   d_entry: device int32[edge_capacity]: the entry's position in the column array, the edge id from
 *     which a caller fetches weights or edge features.
 *   Edges are ordered hop by hop, then by the expanded vertex's local id, then by ascending position.
 *   h_edge_offsets: HOST int64[n_hops + 1]: hop h is [off[h - 1], off[h]).
 * Capacities.  A hop's exact edge count and new-vertex count are known before anything of that hop
 * is written to caller memory (count pass + scan; claim + count).  If a count does not fit, the call
 * returns GRX_ERR_RUNTIME and the message names the hop and the number needed; earlier hops' outputs
 * stay as written.  Bounds that never fail: E_h <= min(|level h - 1| * k_h, nnz), <= nnz for
 * k_h == -1; the sum of E_h over all hops <= nnz (a row is expanded once); nodes <= min(distinct
 * seeds + edges, V).
 * Errors, all found on the host before anything is launched: GRX_ERR_INVALID_ARGUMENT for a NULL ctx,
 * g or h_fanouts, n_seeds < 0, h_seeds == NULL with n_seeds != 0, a seed out of range, n_hops outside
 * [1, 64], a bad fan-out, n_rows != n_cols, a negative capacity, all six outputs NULL, and
 * opt->max_iterations != 0.  opt may be NULL; only collect_kernel_time is read.
 * Method, per hop: a count pass over the frontier (min(d, k) per row, and the row's lane-group class)
 * and a scan; the sampler, one group of 8 lanes, a wavefront or a workgroup per row (all-rows by d,
 * picking rows by m; GRX_SAMPLE_GROUP = 8, 64 or 256 forces one width, 0 = by the rule: an
 * environment variable read per call, a test hook; neither the answer nor the stats defined below
 * depend on it): a group draws a group-width of candidates at once into an LDS open-addressing table
 * of >= 2m slots and decides first occurrences and A in attempt order; discovery (claim
 * local[u] == -1 by compare-and-swap, sort the claimed ids, assign local ids); and the fill of the
 * caller's arrays.  Two host hand-offs per hop.
 * stats may be NULL; set, and defined by the answer: iterations (hops that expanded at least one
 * vertex), vertices_reached (nodes), edges_traversed (sampled edges), edges_expanded (the sum over
 * expanded rows of A, counting d for an all-row), levels_recorded (n_hops), frontier_slots[h - 1]
 * (vertices expanded in hop h); and, defined by the schedule, elapsed_ms, advance_kernel_ms (when
 * collect_kernel_time is set) and advance_launches (this library's kernels).
 * The workspace is released on return and nothing is left on the handle: 4 bytes per vertex for the
 * local-id map (set to -1 per call) and 4 per vertex of the current level; per hop 13 bytes per
 * frontier row (count, offset, order, two class bytes), 12 per sampled edge of the hop and 8 per
 * vertex the hop can still discover (min(E_h, V - nodes)), plus rocPRIM's scan and sort storage. */
int grx_neighbor_sample(grx_context_t ctx, grx_graph_t g, const int32_t* h_seeds, int32_t n_seeds,
                        const int32_t* h_fanouts, int32_t n_hops, uint64_t seed, int32_t* d_nodes,
                        int64_t node_capacity, int32_t* d_src, int32_t* d_dst, int32_t* d_entry,
                        int64_t edge_capacity, int64_t* h_node_offsets, int64_t* h_edge_offsets,
                        const grx_options* opt, grx_stats* stats);

/* ---- operators (frontier-level overloads) -------------------------------- */
/* operators::advance::execute<lb, forward, in, out>(G, op, input, output, segments, context)
 * (framework/operators/advance/advance.hxx:91-129).
 *   d_input == NULL  -> advance_io_type_t::graph (all n_rows vertices)
 *   d_output == NULL -> advance_io_type_t::none
 * *n_output receives the new number of elements; the output holds them in unspecified
 * order (block_mapped.hxx:94-101). Fails with GRX_ERR_RUNTIME if output_capacity is too small. */
int grx_advance(grx_context_t ctx, grx_graph_t g, const grx_options* opt, int32_t edge_op,
                void* d_state, int32_t iparam, const int32_t* d_input, int64_t n_input,
                int32_t* d_output, int64_t output_capacity, int64_t* n_output);
/* operators::filter::execute<alg>(G, op, input, output, context)  filter/filter.hxx:59-86 */
int grx_filter(grx_context_t ctx, grx_graph_t g, int32_t algorithm, int32_t vertex_op,
               void* d_state, int32_t iparam, const int32_t* d_input, int64_t n_input,
               int32_t* d_output, int64_t output_capacity, int64_t* n_output);
/* operators::uniquify::execute<alg>(input, output, context, best_effort)  uniquify.hxx:15-42.
 * GRX_UNIQUE leaves the result in d_input (d_output is scratch of >= n_input elements). */
int grx_uniquify(grx_context_t ctx, int32_t algorithm, int32_t best_effort, int32_t* d_input,
                 int64_t n_input, int32_t* d_output, int64_t output_capacity, int64_t* n_output);

/* ---- multi-GPU: one process per GPU, frontier all-gather over RCCL/xGMI ------------------ */
/* The reference declares multi_context_t for several devices but every operator throws for
 * size() != 1 (advance.hxx:125-128); this is new functionality.
 *
 * Model: 1-D vertex partition.  Rank r owns rows [row_begin,row_end); its local CSR keeps GLOBAL
 * vertex ids and has all V rows, the rows it does not own being empty.  Every rank holds a
 * replica of the label array (BFS depth / SSSP distance).  One BSP superstep =
 *   grx_partitioned_expand   local advance over the owned input frontier (any schedule) with the
 *                            BFS / SSSP functor on the replica; the vertices it improved are
 *                            packed as [count | (vertex,label) ...] into the rank's send slot
 *   all-gather of the send slots over RCCL (done by the host: torch.distributed / ncclAllGather)
 *   grx_partitioned_admit    min-combine every other rank's pairs into the replica and append
 *                            the owned, improved vertices to the next input frontier
 * Dense BFS supersteps (more finds than V/64) exchange per-rank LEVEL BITMAPS instead of pairs
 * (grx_partitioned_level_bitmap + recv_format GRX_RECV_LEVEL_BITMAP).
 * grx_partitioned_run (below) is the whole loop in C++ with the collectives issued directly on
 * RCCL; the step-level entry points stay public for hosts that bring their own loop. */

/* Rank-local slice of a replicated graph; split points balance EDGES (prefix of row offsets). */
int grx_graph_partition(grx_graph_t full, int rank, int world_size, grx_graph_t* out,
                        int32_t* row_begin, int32_t* row_end);
/* The same slice of the graph's HOT-FIRST renumbered copy (grx_graph_hot_first; built here if the
 * handle has none yet): [row_begin, row_end) is then a range of RENUMBERED vertices (edge-balanced
 * like above: the first ranks own few, heavy vertices), and the slice remembers both permutations.
 * grx_partitioned_run on a plan made from it takes the source and delivers the labels in the
 * CALLER's numbering (sources in, labels out, as for grx_bfs): the supersteps run on renumbered
 * replicas, one scatter pass at the end of the run writes d_labels.  The single-superstep entry
 * points below (grx_partitioned_expand / _admit / _step) see such a slice as the plain graph it is --
 * renumbered ids in and out. */
int grx_graph_partition_hot_first(grx_context_t ctx, grx_graph_t full, int rank, int world_size,
                                  grx_graph_t* out, int32_t* row_begin, int32_t* row_end);
/* d_labels: replica [V] (int32 depth for GRX_OP_BFS, float distance for GRX_OP_SSSP).
 * round: superstep number (the BFS level).  d_frontier / n_frontier: owned input frontier
 * (global ids).  d_scratch: int32[scratch_capacity] workspace for the raw output frontier
 * (>= sum of degrees of the frontier; local nnz + V is enough for a duplicate-free frontier).
 * d_sent_stamp: int32[V], -1 initially: a vertex improved several times in one superstep is
 * packed once.  d_send: int64[send_capacity >= V + 1]; word 0 receives the number of pairs,
 * words 1.. the pairs (low 32 bits vertex, high 32 bits label bits).  *n_found = that count. */
int grx_partitioned_expand(grx_context_t ctx, grx_graph_t local, const grx_options* opt,
                           int32_t edge_op, void* d_labels, int32_t round,
                           const int32_t* d_frontier, int64_t n_frontier, int32_t* d_scratch,
                           int64_t scratch_capacity, int32_t* d_sent_stamp, int64_t* d_send,
                           int64_t send_capacity, int64_t* n_found);
/* What a gathered buffer holds. */
typedef enum grx_recv_format {
  GRX_RECV_PAIRS = 0,        /* per rank: [count | (vertex,label) ...], `slot` words each           */
  GRX_RECV_LEVEL_BITMAP = 1, /* BFS only, dense supersteps: per rank ceil(V/64) words, bit v = "this
                                rank discovered v in the superstep"; labels are implied (the level) */
  GRX_RECV_REPLICA_MIN = 2   /* dense SSSP supersteps: nothing was gathered -- the host all-reduced
                                (MIN) the label replicas in place; d_recv is the label SNAPSHOT
                                (one entry per vertex) grx_partitioned_step took before the advance:
                                owned vertices whose label fell below it are admitted             */
} grx_recv_format;

/* Dense BFS exchange, enqueue-only: d_words[ceil(V/64)] <- bit v = (d_depth[v] == level).  Called
 * after a superstep whose finds (level = round + 1) are too many for the pair list: V/8 bytes per
 * rank travel instead of 8 bytes per discovery. */
int grx_partitioned_level_bitmap(grx_context_t ctx, const int32_t* d_depth, int64_t n_vertices,
                                 int32_t level, int64_t* d_words, int64_t word_capacity);

/* d_recv: int64[world_size * slot] gathered send slots (recv_format says what they hold).
 * GRX_RECV_PAIRS: pairs of other ranks are min-combined into d_labels; a vertex is appended to
 * d_next (capacity next_capacity) when it is owned (row_begin <= v < row_end), its label improved
 * (or it is one of this rank's own discoveries) and d_stamp[v] != round (then d_stamp[v] = round:
 * one copy per superstep, like the bypass filter of reference algorithms/sssp.hxx:126-136).
 * GRX_RECV_LEVEL_BITMAP: every vertex in the union of the bitmaps gets depth round + 1; the owned
 * ones are appended (ascending).  `round` = the superstep whose finds were gathered. */
int grx_partitioned_admit(grx_context_t ctx, int32_t edge_op, void* d_labels, int64_t n_vertices,
                          int32_t* d_stamp, int32_t round, const int64_t* d_recv,
                          int32_t recv_format, int32_t world_size, int64_t slot, int32_t my_rank,
                          int32_t row_begin, int32_t row_end, int32_t* d_next,
                          int64_t next_capacity, int64_t* n_next);

/* The same superstep FUSED and enqueue-only (block_mapped schedule): [admit d_recv, the gather of
 * superstep round - 1, into d_frontier / *d_frontier_count ->] advance over d_frontier (its length
 * is read on the DEVICE from *d_frontier_count) -> pack into d_send.  Nothing is awaited: the
 * caller issues the collective on the SAME stream (create the context on that stream) and
 * synchronises once per superstep, on the gathered counts.  d_recv == NULL on the first superstep
 * (the caller preset d_frontier / *d_frontier_count).  Buffer overflows of a step are reported by
 * the next call.  d_snapshot (optional, 4 bytes per vertex): receives the labels of the owned range
 * as they are before the advance, for a GRX_RECV_REPLICA_MIN admission by the next call. */
int grx_partitioned_step(grx_context_t ctx, grx_graph_t local, const grx_options* opt,
                         int32_t edge_op, void* d_labels, int32_t* d_stamp, int32_t* d_sent_stamp,
                         int32_t round, const int64_t* d_recv, int32_t recv_format,
                         int32_t world_size, int64_t slot, int32_t my_rank, int32_t row_begin,
                         int32_t row_end, int32_t* d_frontier, int64_t frontier_capacity,
                         uint64_t* d_frontier_count, int32_t* d_scratch, int64_t scratch_capacity,
                         int64_t* d_send, int64_t send_capacity, void* d_snapshot);

/* PageRank on the same partition (replicas of the rank vector p): one iteration's
 * local half.  d_partial[V + 1] <- contributions of the rows this rank owns,
 *   d_partial[dst] += d_rank[src] * d_scale[src] * w   over the local edges   (pr.hxx:140-146)
 *   d_partial[V]    = alpha * (sum of d_rank over the OWNED vertices without out-edges)
 * d_scale[V] (alpha / sum of out-weights, 0 for rows without edges; pr.hxx:77-91) is computed when
 * compute_scale != 0 and reused otherwise.  The host all-reduces d_partial (SUM) and sets
 *   p[v] = (1 - alpha + partial[V]) / V + partial[v];  done when max |p - p_previous| < tol.
 * Synchronous. */
int grx_pagerank_partitioned_scatter(grx_context_t ctx, grx_graph_t local, float alpha,
                                     const float* d_rank, float* d_scale, int32_t compute_scale,
                                     float* d_partial, int32_t row_begin, int32_t row_end,
                                     const grx_options* opt);

/* ---- multi-GPU: the job, and the whole traversal as ONE call -------------------------------- */
/* A context joins a job of `world_size` ranks (one process per GPU; this IS
 * gcuda::multi_context_t::attach_job).  Two transports:
 *   grx_context_attach_rccl         RCCL over xGMI (production): ncclCommInitRank with the 128-byte
 *                                   id rank 0 obtained from grx_job_unique_id and handed to the
 *                                   other ranks by any side channel; collective over all ranks.
 *                                   ncclAllGather / ncclAllReduce are then issued by the C++
 *                                   superstep loop on the context's own stream.
 *   grx_context_attach_collectives  host callbacks with the same meaning (device pointers in,
 *                                   device pointers out; the callback may stage through the host
 *                                   but must have completed when it returns).  For transports
 *                                   other than RCCL and for test rigs (ranks sharing one GPU). */
#define GRX_UNIQUE_ID_BYTES 128
typedef enum grx_collective_dtype { GRX_INT32 = 0, GRX_FLOAT32 = 1, GRX_INT64 = 2 } grx_collective_dtype;
typedef enum grx_collective_op { GRX_MIN = 0, GRX_SUM = 1, GRX_MAX = 2 } grx_collective_op;
typedef int (*grx_all_gather_fn)(void* user, const void* d_send, void* d_recv,
                                 uint64_t bytes_per_rank, void* stream);
typedef int (*grx_all_reduce_fn)(void* user, void* d_buffer, uint64_t count, int32_t dtype,
                                 int32_t op, void* stream);
int grx_job_unique_id(void* id128);
int grx_context_attach_rccl(grx_context_t ctx, int rank, int world_size, const void* id128);
int grx_context_attach_collectives(grx_context_t ctx, int rank, int world_size,
                                   grx_all_gather_fn all_gather, grx_all_reduce_fn all_reduce,
                                   void* user);
int grx_context_detach(grx_context_t ctx);
/* backend: "single" (no job), "rccl" or "hooks". */
int grx_context_job_info(grx_context_t ctx, int32_t* rank, int32_t* world_size, char* backend,
                         size_t backend_len);

/* A partitioned traversal's persistent state: the rank's slice, its owned range and every buffer
 * the supersteps need (frontier, raw output, send / receive slots, level bitmaps, stamps), all
 * allocated once.  small_slot: int64 words per rank in the first all-gather of a superstep
 * (0 = 32768, i.e. 256 KiB); dense_threshold / replica_threshold: finds on the busiest rank
 * above which BFS exchanges level bitmaps / SSSP all-reduces the replicas (0 = V/64 and
 * V/world_size; negative = never). */
typedef struct grx_partitioned_s* grx_partitioned_t;
typedef struct grx_partitioned_stats {
  float elapsed_ms;             /* host wall time of the superstep loop (device drained)        */
  int32_t supersteps;
  int32_t collectives;          /* all-gathers + all-reduces issued by this rank                 */
  int32_t bitmap_supersteps;    /* BFS supersteps that exchanged level bitmaps                   */
  int32_t allreduce_supersteps; /* SSSP supersteps that all-reduced (MIN) the replicas           */
  int32_t iterations;           /* PageRank: iterations                                          */
  float last_error;             /* PageRank: max |p - p_previous| of the last iteration          */
  int64_t pairs_exchanged;      /* finds of all ranks over the run                               */
  int64_t bytes_sent;           /* payload bytes this rank contributed to collectives            */
  int32_t large_gather_supersteps; /* supersteps whose pairs outgrew the first (small) slot: one
                                      more all-gather; collectives == supersteps + bitmap_ +
                                      allreduce_ + large_gather_supersteps for a traversal        */
  int32_t reserved;
} grx_partitioned_stats;
int grx_partitioned_create(grx_context_t ctx, grx_graph_t local, int32_t row_begin, int32_t row_end,
                           const grx_options* opt, int64_t small_slot, int64_t dense_threshold,
                           int64_t replica_threshold, grx_partitioned_t* out);
int grx_partitioned_destroy(grx_partitioned_t plan);
/* The whole BSP loop in C++ (what essentials_amd/distributed.py drove from Python in round 1):
 * reset the replica and the stamps, then per superstep ONE enqueue-only grx_partitioned_step, the
 * all-gather of the send slots on the SAME stream, one host wait on the gathered counts, and --
 * by the busiest rank's count -- the level-bitmap all-gather (BFS), the replica all-reduce (SSSP)
 * or a second, larger all-gather.  edge_op: GRX_OP_BFS (d_labels int32[V]) or GRX_OP_SSSP
 * (float[V]); every rank passes the same source and gets the full label array.  Collective over
 * the job the context is attached to (a context without a job runs it as a job of one). */
int grx_partitioned_run(grx_partitioned_t plan, int32_t edge_op, int32_t source, void* d_labels,
                        grx_partitioned_stats* stats);
/* PageRank on the same plan: per iteration the local scatter (grx_pagerank_partitioned_scatter),
 * ONE all-reduce (SUM) of V + 1 floats, the update and the stop test
 * max |p - p_previous| < tol after >= 1 iteration (pr.hxx:155-178); max_iterations 0 = none. */
int grx_partitioned_pagerank(grx_partitioned_t plan, float alpha, float tol, int32_t max_iterations,
                             float* d_p, grx_partitioned_stats* stats);

/* ---- measurement helpers ------------------------------------------------- */
/* Streaming copy of `bytes` (16 B per lane) timed with events on the context stream:
 * the achievable-HBM roof quoted beside the 8 TB/s vendor peak. Returns GB/s. */
int grx_measure_copy_bandwidth(grx_context_t ctx, size_t bytes, int repeats, double* gbps);

/* Random-gather ceiling of a graph: acc += table[column_indices[i]] over ALL its edges (4-B table
 * entries, one per vertex) -- the access every label-testing advance functor shares (reference
 * bfs.hxx:92-107, sssp.hxx:95-113), without frontier logic, atomics or output.  mode 0 = plain
 * (L1-cached) loads, 1 = the agent-scope loads math::atomic::min pre-tests with.  Best of
 * `repeats`; returns lookups (= edges) per second: the roof MTEPS of a push traversal is
 * measured against. */
int grx_measure_gather_rate(grx_context_t ctx, grx_graph_t g, int mode, int repeats,
                            double* lookups_per_second);

#ifdef __cplusplus
}
#endif
#endif /* ESSENTIALS_AMD_H */

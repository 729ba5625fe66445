"""ctypes binding of include/essentials_amd.h and a small object layer over it.

Names follow the reference's domain (graph, frontier, advance, filter, enactor stats).
Mirrors, argument for argument, ``gunrock::{bfs,sssp,pr}::run`` (reference
algorithms/bfs.hxx:151-176, sssp.hxx:155-185, pr.hxx:182-216) and the frontier-level
operator overloads (advance.hxx:91-129, filter.hxx:59-86, uniquify.hxx:15-42).
"""
from __future__ import annotations

import ctypes as C
import enum
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# ESSENTIALS_AMD_LIB selects an experiment build of the SAME library (see build.build_variant)
_LIB_PATH = os.environ.get("ESSENTIALS_AMD_LIB") or os.path.join(_PKG, "libessentials_amd.so")

INT_UNREACHED = 2**31 - 1
FLT_UNREACHED = float(np.finfo(np.float32).max)


class EngineError(RuntimeError):
    """A C-ABI call failed (the C++ surface threw gunrock::error::exception_t).  `code` is the
    grx_status: -1 invalid argument, -2 runtime, -3 unsupported, -4 a peer rank's superstep failed,
    -5 a superstep's gather timed out (exit without synchronising the context)."""
    code = 0


ERR_PEER, ERR_TIMEOUT = -4, -5


class LoadBalance(enum.IntEnum):
    thread_mapped = 0
    warp_mapped = 1
    block_mapped = 2
    bucketing = 3
    merge_path = 4
    merge_path_v2 = 5
    work_stealing = 6


class FilterAlgorithm(enum.IntEnum):
    remove = 0
    predicated = 1
    compact = 2
    bypass = 3


class UniquifyAlgorithm(enum.IntEnum):
    unique = 0
    unique_copy = 1


class EdgeOp(enum.IntEnum):
    all = 0
    bfs = 1
    sssp = 2
    count_edge = 3
    sum_weight = 4


class VertexOp(enum.IntEnum):
    all = 0
    odd = 1
    once = 2
    count = 3


class _Options(C.Structure):
    _fields_ = [("load_balance", C.c_int32), ("holes_layout", C.c_int32),
                ("hub_threshold", C.c_int32), ("max_iterations", C.c_int32),
                ("frontier_sizing_factor", C.c_float), ("collect_kernel_time", C.c_int32),
                ("chunk_edges", C.c_int32), ("direction_optimized", C.c_int32),
                ("do_alpha", C.c_float), ("do_beta", C.c_float),
                ("chunk_queue_limit", C.c_int32), ("sssp_two_pass", C.c_int32),
                ("call_every_edge", C.c_int32)]


class _Stats(C.Structure):
    _fields_ = [("elapsed_ms", C.c_float), ("advance_kernel_ms", C.c_float),
                ("iterations", C.c_int32), ("advance_launches", C.c_int32),
                ("vertices_reached", C.c_int64), ("edges_traversed", C.c_int64),
                ("levels_recorded", C.c_int32), ("pull_iterations", C.c_int32),
                ("frontier_slots", C.c_int64 * 64), ("edges_expanded", C.c_int64)]


class _PartitionedStats(C.Structure):
    _fields_ = [("elapsed_ms", C.c_float), ("supersteps", C.c_int32), ("collectives", C.c_int32),
                ("bitmap_supersteps", C.c_int32), ("allreduce_supersteps", C.c_int32),
                ("iterations", C.c_int32), ("last_error", C.c_float),
                ("pairs_exchanged", C.c_int64), ("bytes_sent", C.c_int64),
                ("large_gather_supersteps", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


# collective callbacks of grx_context_attach_collectives
ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)
ALL_REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32,
                            C.c_void_p)
UNIQUE_ID_BYTES = 128


@dataclass
class Options:
    load_balance: LoadBalance = LoadBalance.block_mapped
    holes_layout: bool = False
    hub_threshold: int = 0
    max_iterations: int = 0
    frontier_sizing_factor: float = 1.5
    collect_kernel_time: bool = False
    chunk_edges: int = 0
    direction_optimized: bool = False
    do_alpha: float = 0.0
    do_beta: float = 0.0
    chunk_queue_limit: int = 0
    sssp_two_pass: bool = False
    call_every_edge: bool = False

    def _c(self) -> _Options:
        o = _Options()
        o.load_balance = int(self.load_balance)
        o.holes_layout = int(self.holes_layout)
        o.hub_threshold = int(self.hub_threshold)
        o.max_iterations = int(self.max_iterations)
        o.frontier_sizing_factor = float(self.frontier_sizing_factor)
        o.collect_kernel_time = int(self.collect_kernel_time)
        o.chunk_edges = int(self.chunk_edges)
        o.direction_optimized = int(self.direction_optimized)
        o.do_alpha = float(self.do_alpha)
        o.do_beta = float(self.do_beta)
        o.chunk_queue_limit = int(self.chunk_queue_limit)
        o.sssp_two_pass = int(self.sssp_two_pass)
        o.call_every_edge = int(self.call_every_edge)
        return o


@dataclass
class Stats:
    elapsed_ms: float = 0.0
    advance_kernel_ms: float = 0.0
    iterations: int = 0
    advance_launches: int = 0
    vertices_reached: int = 0
    edges_traversed: int = 0
    frontier_slots: list = field(default_factory=list)
    pull_iterations: int = 0
    edges_expanded: int = 0

    @staticmethod
    def _from(s: _Stats) -> "Stats":
        return Stats(s.elapsed_ms, s.advance_kernel_ms, s.iterations, s.advance_launches,
                     s.vertices_reached, s.edges_traversed,
                     list(s.frontier_slots[: s.levels_recorded]), s.pull_iterations,
                     s.edges_expanded)


# symbol -> (restype, argtypes); the list is also what tests check against the header
_VP = C.c_void_p
_SIGNATURES = {
    "grx_abi_version": (C.c_int, []),
    "grx_last_error": (C.c_char_p, []),
    "grx_default_options": (None, [C.POINTER(_Options)]),
    "grx_context_create": (C.c_int, [C.c_int, _VP, C.POINTER(_VP)]),
    "grx_context_destroy": (C.c_int, [_VP]),
    "grx_context_synchronize": (C.c_int, [_VP]),
    "grx_context_wait_stream": (C.c_int, [_VP, _VP]),
    "grx_trim_cache": (C.c_int, []),
    "grx_copy_to_host": (C.c_int, [_VP, _VP, _VP, C.c_size_t]),
    "grx_copy_to_device": (C.c_int, [_VP, _VP, _VP, C.c_size_t]),
    "grx_job_unique_id": (C.c_int, [_VP]),
    "grx_context_attach_rccl": (C.c_int, [_VP, C.c_int, C.c_int, _VP]),
    "grx_context_attach_collectives": (C.c_int, [_VP, C.c_int, C.c_int, _VP, _VP, _VP]),
    "grx_context_detach": (C.c_int, [_VP]),
    "grx_context_job_info": (C.c_int, [_VP, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p,
                                       C.c_size_t]),
    "grx_partitioned_create": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.POINTER(_Options),
                                         C.c_int64, C.c_int64, C.c_int64, C.POINTER(_VP)]),
    "grx_partitioned_destroy": (C.c_int, [_VP]),
    "grx_partitioned_run": (C.c_int, [_VP, C.c_int32, C.c_int32, _VP, C.POINTER(_PartitionedStats)]),
    "grx_partitioned_pagerank": (C.c_int, [_VP, C.c_float, C.c_float, C.c_int32, _VP,
                                           C.POINTER(_PartitionedStats)]),
    "grx_context_device_info": (C.c_int, [_VP, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int64), C.c_char_p, C.c_size_t]),
    "grx_graph_from_device_csr": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP,
                                            C.POINTER(_VP)]),
    "grx_graph_from_host_csr": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP,
                                          C.POINTER(_VP)]),
    "grx_graph_from_mtx": (C.c_int, [C.c_char_p, C.POINTER(_VP)]),
    "grx_graph_from_csr_file": (C.c_int, [C.c_char_p, C.POINTER(_VP)]),
    "grx_graph_write_csr_file": (C.c_int, [_VP, C.c_char_p]),
    "grx_graph_rmat": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int,
                                 C.POINTER(_VP)]),
    "grx_graph_sorted_rows": (C.c_int, [_VP, _VP, C.POINTER(_VP)]),
    "grx_graph_simple": (C.c_int, [_VP, _VP, C.POINTER(_VP)]),
    "grx_graph_build_in_edges": (C.c_int, [_VP, _VP]),
    "grx_graph_hot_first": (C.c_int, [_VP, _VP, C.c_int]),
    "grx_graph_destroy": (C.c_int, [_VP]),
    "grx_graph_info": (C.c_int, [_VP, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int64), C.POINTER(_VP), C.POINTER(_VP),
                                 C.POINTER(_VP)]),
    "grx_graph_copy_to_host": (C.c_int, [_VP, _VP, _VP, _VP]),
    "grx_bfs": (C.c_int, [_VP, _VP, C.c_int32, _VP, _VP, C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_sssp": (C.c_int, [_VP, _VP, C.c_int32, _VP, _VP, C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_pagerank": (C.c_int, [_VP, _VP, C.c_float, C.c_float, _VP, C.POINTER(_Options),
                               C.POINTER(_Stats)]),
    "grx_bc": (C.c_int, [_VP, _VP, _VP, C.c_int32, _VP, C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_tc": (C.c_int, [_VP, _VP, _VP, C.POINTER(C.c_uint64), C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_kcore": (C.c_int, [_VP, _VP, _VP, C.POINTER(C.c_int32), C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_color": (C.c_int, [_VP, _VP, _VP, C.POINTER(C.c_int32), C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_cc": (C.c_int, [_VP, _VP, _VP, C.POINTER(C.c_int64), C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_scc": (C.c_int, [_VP, _VP, _VP, C.POINTER(C.c_int64), C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_lpa": (C.c_int, [_VP, _VP, _VP, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(_Options),
                          C.POINTER(_Stats)]),
    "grx_louvain": (C.c_int, [_VP, _VP, _VP, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                              C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_modularity": (C.c_int, [_VP, _VP, _VP, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                 C.POINTER(C.c_uint64), C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_mst": (C.c_int, [_VP, _VP, _VP, C.POINTER(C.c_int64), C.POINTER(C.c_double), _VP,
                          C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_spgemm": (C.c_int, [_VP, _VP, _VP, C.POINTER(_VP), C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_truss": (C.c_int, [_VP, _VP, _VP, C.POINTER(C.c_int32), C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_bfs_multi": (C.c_int, [_VP, _VP, _VP, C.c_int32, _VP, _VP, _VP, _VP, C.POINTER(_Options),
                                C.POINTER(_Stats)]),
    "grx_ppr": (C.c_int, [_VP, _VP, _VP, C.c_int32, C.c_float, C.c_float, _VP, _VP, _VP, C.POINTER(_Options),
                          C.POINTER(_Stats)]),
    "grx_spmv": (C.c_int, [_VP, _VP, C.c_int32, _VP, _VP, C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_spmm": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int64, _VP, C.c_int64, C.POINTER(_Options),
                           C.POINTER(_Stats)]),
    "grx_spmm_values": (C.c_int, [_VP, _VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int64, _VP, C.c_int64,
                                  C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_sddmm": (C.c_int, [_VP, _VP, C.c_int32, _VP, C.c_int64, _VP, C.c_int64, _VP, C.POINTER(_Options),
                            C.POINTER(_Stats)]),
    "grx_edge_softmax": (C.c_int, [_VP, _VP, C.c_int32, _VP, _VP, C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_edge_softmax_backward": (C.c_int, [_VP, _VP, C.c_int32, _VP, _VP, _VP, C.POINTER(_Options),
                                            C.POINTER(_Stats)]),
    "grx_hits": (C.c_int, [_VP, _VP, C.c_float, _VP, _VP, C.POINTER(C.c_int32), C.POINTER(C.c_float),
                           C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_bfs_predecessors": (C.c_int, [_VP, _VP, C.c_int32, _VP, _VP, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                       C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_sssp_predecessors": (C.c_int, [_VP, _VP, C.c_int32, _VP, _VP, _VP, C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int64), C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_random_walk": (C.c_int, [_VP, _VP, _VP, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_float, C.c_float,
                                  _VP, C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_neighbor_sample": (C.c_int, [_VP, _VP, _VP, C.c_int32, _VP, C.c_int32, C.c_uint64, _VP, C.c_int64, _VP, _VP,
                                      _VP, C.c_int64, _VP, _VP, C.POINTER(_Options), C.POINTER(_Stats)]),
    "grx_advance": (C.c_int, [_VP, _VP, C.POINTER(_Options), C.c_int32, _VP, C.c_int32, _VP,
                              C.c_int64, _VP, C.c_int64, C.POINTER(C.c_int64)]),
    "grx_filter": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP, C.c_int32, _VP, C.c_int64, _VP,
                             C.c_int64, C.POINTER(C.c_int64)]),
    "grx_uniquify": (C.c_int, [_VP, C.c_int32, C.c_int32, _VP, C.c_int64, _VP, C.c_int64,
                               C.POINTER(C.c_int64)]),
    "grx_graph_partition": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(_VP), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32)]),
    "grx_graph_partition_hot_first": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.POINTER(_VP),
                                                C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "grx_partitioned_expand": (C.c_int, [_VP, _VP, C.POINTER(_Options), C.c_int32, _VP, C.c_int32,
                                         _VP, C.c_int64, _VP, C.c_int64, _VP, _VP, C.c_int64,
                                         C.POINTER(C.c_int64)]),
    "grx_partitioned_level_bitmap": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, _VP, C.c_int64]),
    "grx_partitioned_admit": (C.c_int, [_VP, C.c_int32, _VP, C.c_int64, _VP, C.c_int32, _VP,
                                        C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                        C.c_int32, _VP, C.c_int64, C.POINTER(C.c_int64)]),
    "grx_partitioned_step": (C.c_int, [_VP, _VP, C.POINTER(_Options), C.c_int32, _VP, _VP, _VP,
                                       C.c_int32, _VP, C.c_int32, C.c_int32, C.c_int64, C.c_int32,
                                       C.c_int32, C.c_int32, _VP, C.c_int64, _VP, _VP, C.c_int64,
                                       _VP, C.c_int64, _VP]),
    "grx_pagerank_partitioned_scatter": (C.c_int, [_VP, _VP, C.c_float, _VP, _VP, C.c_int32, _VP,
                                                   C.c_int32, C.c_int32, C.POINTER(_Options)]),
    "grx_measure_copy_bandwidth": (C.c_int, [_VP, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    "grx_measure_gather_rate": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.POINTER(C.c_double)]),
}

_lib = None


def library_path() -> str:
    return _LIB_PATH


def load_library():
    """Load libessentials_amd.so; there is no fallback of any kind."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise EngineError(
            f"{_LIB_PATH} is missing: build it with `python -m essentials_amd.build` "
            "(hipcc --offload-arch=gfx950). essentials_amd has no CPU path.")
    # torch ships its own copy of the HIP runtime (same SONAME as /opt/rocm's): load torch's
    # first so that this process has ONE runtime -- with the order reversed torch later fails
    # with "No HIP GPUs are available".
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(_LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.grx_abi_version() != 1:
        raise EngineError("ABI version mismatch")
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load_library().grx_last_error()
        err = EngineError(f"{what} failed ({rc}): {msg.decode(errors='replace') if msg else ''}")
        err.code = rc
        raise err


def _ptr(t) -> Optional[int]:
    """Device (torch) or host (numpy) pointer of an array-like, None -> NULL."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return t.ctypes.data
    return t.data_ptr()


class Context:
    """gcuda::multi_context_t(device[, stream])  (reference cuda/context.hxx:136-206)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self._h = _VP()
        _check(load_library().grx_context_create(device, stream, C.byref(self._h)),
               "grx_context_create")
        self.device = device
        self._stream = stream   # None: the engine's private non-blocking stream

    def synchronize(self) -> None:
        _check(load_library().grx_context_synchronize(self._h), "grx_context_synchronize")

    def after_torch(self) -> None:
        """Order the engine's next work after everything torch has enqueued on ITS current stream
        of this device (event record + stream wait on the device; the host does not wait).  A
        default Context runs on a private non-blocking stream that is ordered after nothing:
        tensors a caller has just filled (`torch.full`, `clone`, `copy_`) must not be read by an
        engine kernel before the fill has run.  Every wrapper below that takes tensors calls this;
        it is a no-op when the context was created on torch's current stream."""
        import torch
        if not torch.cuda.is_available():
            return
        cur = torch.cuda.current_stream(self.device).cuda_stream
        if self._stream is not None and cur == self._stream:
            return
        _check(load_library().grx_context_wait_stream(self._h, cur), "grx_context_wait_stream")

    def device_info(self) -> dict:
        cus, wave, mem = C.c_int32(), C.c_int32(), C.c_int64()
        name = C.create_string_buffer(256)
        _check(load_library().grx_context_device_info(self._h, cus, wave, mem, name, 256),
               "grx_context_device_info")
        return {"name": name.value.decode(), "compute_units": cus.value,
                "wavefront_size": wave.value, "total_memory_bytes": mem.value}

    def copy_bandwidth_gbps(self, nbytes: int = 1 << 30, repeats: int = 10) -> float:
        g = C.c_double()
        _check(load_library().grx_measure_copy_bandwidth(self._h, nbytes, repeats, g),
               "grx_measure_copy_bandwidth")
        return g.value

    # -- multi-GPU job (gcuda::multi_context_t::attach_job) ---------------------------------
    def attach_rccl(self, rank: int, world: int, unique_id: bytes) -> None:
        """Join an RCCL job: ncclCommInitRank with the id rank 0 got from Context.unique_id().
        Collective over all ranks."""
        assert len(unique_id) == UNIQUE_ID_BYTES
        buf = C.create_string_buffer(unique_id, UNIQUE_ID_BYTES)
        _check(load_library().grx_context_attach_rccl(self._h, rank, world, buf),
               "grx_context_attach_rccl")

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(UNIQUE_ID_BYTES)
        _check(load_library().grx_job_unique_id(buf), "grx_job_unique_id")
        return buf.raw

    def attach_collectives(self, rank: int, world: int, all_gather, all_reduce) -> None:
        """Join a job whose collectives are host callbacks:
        all_gather(d_send: int, d_recv: int, bytes_per_rank: int, stream: int) -> int (0 = ok) and
        all_reduce(d_buffer: int, count: int, dtype: int, op: int, stream: int) -> int."""
        def _ag(_user, send, recv, nbytes, stream):
            try:
                return int(all_gather(send, recv, nbytes, stream) or 0)
            except Exception as e:   # an exception must not unwind through the C frames
                print(f"[essentials_amd] all_gather callback failed: {e!r}", flush=True)
                return -1

        def _ar(_user, buf, count, dtype, op, stream):
            try:
                return int(all_reduce(buf, count, dtype, op, stream) or 0)
            except Exception as e:
                print(f"[essentials_amd] all_reduce callback failed: {e!r}", flush=True)
                return -1
        self._callbacks = (ALL_GATHER_FN(_ag), ALL_REDUCE_FN(_ar))   # keep them alive
        _check(load_library().grx_context_attach_collectives(
            self._h, rank, world, C.cast(self._callbacks[0], _VP), C.cast(self._callbacks[1], _VP),
            None), "grx_context_attach_collectives")

    def detach(self) -> None:
        _check(load_library().grx_context_detach(self._h), "grx_context_detach")
        self._callbacks = None

    def job_info(self) -> dict:
        r, w = C.c_int32(), C.c_int32()
        name = C.create_string_buffer(32)
        _check(load_library().grx_context_job_info(self._h, r, w, name, 32), "grx_context_job_info")
        return {"rank": r.value, "world_size": w.value, "backend": name.value.decode()}

    def copy_to_host(self, h_dst: np.ndarray, d_src: int) -> None:
        _check(load_library().grx_copy_to_host(self._h, h_dst.ctypes.data, d_src, h_dst.nbytes),
               "grx_copy_to_host")

    def copy_to_device(self, d_dst: int, h_src: np.ndarray) -> None:
        _check(load_library().grx_copy_to_device(self._h, d_dst, h_src.ctypes.data, h_src.nbytes),
               "grx_copy_to_device")

    @staticmethod
    def trim_cache() -> None:
        """Return the device blocks the engine parked for reuse to the device (see
        grx_trim_cache): for hosts whose OTHER allocator (torch) runs short."""
        _check(load_library().grx_trim_cache(), "grx_trim_cache")

    def gather_rate(self, graph, mode: int = 1, repeats: int = 5) -> float:
        """Random-gather ceiling of `graph` in lookups (= edges) per second: table[column[i]] over
        all edges; mode 1 = the agent-scope loads atomic::min pre-tests with, 0 = plain loads."""
        r = C.c_double()
        _check(load_library().grx_measure_gather_rate(self._h, graph._h, mode, repeats, r),
               "grx_measure_gather_rate")
        return r.value

    def close(self) -> None:
        if self._h:
            load_library().grx_context_destroy(self._h)
            self._h = _VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PartitionedPlan:
    """grx_partitioned_t: the persistent state of vertex-partitioned traversals on one rank and the
    C++ superstep loop over it (grx_partitioned_run / grx_partitioned_pagerank).  The context must
    already be attached to its job (Context.attach_rccl / attach_collectives)."""

    def __init__(self, ctx: Context, local: "Graph", row_begin: int, row_end: int,
                 options: Optional["Options"] = None, small_slot: int = 0, dense_threshold: int = 0,
                 replica_threshold: int = 0):
        self._h = _VP()
        self.ctx, self.local = ctx, local     # keep both alive
        o = (options or Options())._c()
        _check(load_library().grx_partitioned_create(ctx._h, local._h, row_begin, row_end, C.byref(o),
                                                     small_slot, dense_threshold, replica_threshold,
                                                     C.byref(self._h)), "grx_partitioned_create")

    def run(self, op: "EdgeOp", source: int, labels) -> dict:
        """labels: replica [V] (int32 for BFS, float32 for SSSP), overwritten.  Collective."""
        s = _PartitionedStats()
        self.ctx.after_torch()
        _check(load_library().grx_partitioned_run(self._h, int(op), source, _ptr(labels), C.byref(s)),
               "grx_partitioned_run")
        return s.as_dict()

    def pagerank(self, p, alpha: float = 0.85, tol: float = 1e-6, max_iterations: int = 0) -> dict:
        s = _PartitionedStats()
        self.ctx.after_torch()
        _check(load_library().grx_partitioned_pagerank(self._h, alpha, tol, max_iterations, _ptr(p),
                                                       C.byref(s)), "grx_partitioned_pagerank")
        return s.as_dict()

    def close(self) -> None:
        if self._h:
            load_library().grx_partitioned_destroy(self._h)
            self._h = _VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Graph:
    """graph::graph_t over CSR (reference graph/build.hxx:26-36); int32 ids, float weights."""

    def __init__(self, handle, keepalive=None):
        self._h = handle
        self._keep = keepalive
        n, m, nnz = C.c_int32(), C.c_int32(), C.c_int64()
        _check(load_library().grx_graph_info(self._h, n, m, nnz, None, None, None), "grx_graph_info")
        self.n_rows, self.n_cols, self.nnz = n.value, m.value, nnz.value

    @staticmethod
    def from_host_csr(row_offsets, col, val, n_cols=None) -> "Graph":
        ap = np.ascontiguousarray(row_offsets, np.int32)
        aj = np.ascontiguousarray(col, np.int32)
        ax = np.ascontiguousarray(val, np.float32)
        h = _VP()
        n = len(ap) - 1
        _check(load_library().grx_graph_from_host_csr(
            n, n if n_cols is None else n_cols, len(aj), ap.ctypes.data,
            aj.ctypes.data if len(aj) else None, ax.ctypes.data if len(ax) else None, C.byref(h)),
            "grx_graph_from_host_csr")
        return Graph(h)

    @staticmethod
    def from_device_csr(row_offsets, col, val) -> "Graph":
        """Non-owning view over torch int32/int32/float32 device tensors (kept alive here)."""
        h = _VP()
        n = row_offsets.numel() - 1
        # the handle reduces the largest degree from the arrays on first use: they must be complete
        _torch().cuda.current_stream(row_offsets.device).synchronize()
        _check(load_library().grx_graph_from_device_csr(n, n, col.numel(), _ptr(row_offsets),
                                                        _ptr(col), _ptr(val), C.byref(h)),
               "grx_graph_from_device_csr")
        return Graph(h, keepalive=(row_offsets, col, val))

    @staticmethod
    def from_mtx(path: str) -> "Graph":
        h = _VP()
        _check(load_library().grx_graph_from_mtx(path.encode(), C.byref(h)), "grx_graph_from_mtx")
        return Graph(h)

    @staticmethod
    def from_csr_file(path: str) -> "Graph":
        h = _VP()
        _check(load_library().grx_graph_from_csr_file(path.encode(), C.byref(h)),
               "grx_graph_from_csr_file")
        return Graph(h)

    @staticmethod
    def rmat(ctx: Context, scale: int, edge_factor: int = 16, seed: int = 1, weight_seed: int = 0,
             symmetrize: bool = True) -> "Graph":
        h = _VP()
        _check(load_library().grx_graph_rmat(ctx._h, scale, edge_factor, seed, weight_seed,
                                             int(symmetrize), C.byref(h)), "grx_graph_rmat")
        return Graph(h)

    def sorted_rows(self, ctx: "Context") -> "Graph":
        """Same graph, neighbour lists sorted by column id (SuiteSparse-style layout)."""
        h = _VP()
        _check(load_library().grx_graph_sorted_rows(ctx._h, self._h, C.byref(h)),
               "grx_graph_sorted_rows")
        return Graph(h)

    def simple(self, ctx: "Context") -> "Graph":
        """The simple graph under this one: self loops dropped, repeated entries kept once (smallest
        weight of the repeats), rows sorted by column id."""
        h = _VP()
        _check(load_library().grx_graph_simple(ctx._h, self._h, C.byref(h)), "grx_graph_simple")
        return Graph(h)

    def build_in_edges(self, ctx: "Context") -> "Graph":
        """Attach the transpose (in-edges) of a DIRECTED graph: enables pull / direction-optimised BFS."""
        _check(load_library().grx_graph_build_in_edges(ctx._h, self._h), "grx_graph_build_in_edges")
        return self

    def hot_first(self, ctx: "Context", enable: bool = True) -> "Graph":
        """Build now (or drop and disable) the hot-first renumbered copy bfs / sssp run on; labels
        always come back in this graph's own numbering (include/essentials_amd.h)."""
        _check(load_library().grx_graph_hot_first(ctx._h, self._h, int(enable)), "grx_graph_hot_first")
        return self

    def write_csr_file(self, path: str) -> None:
        _check(load_library().grx_graph_write_csr_file(self._h, path.encode()),
               "grx_graph_write_csr_file")

    def to_host(self):
        ap = np.empty(self.n_rows + 1, np.int32)
        aj = np.empty(max(self.nnz, 1), np.int32)
        ax = np.empty(max(self.nnz, 1), np.float32)
        _check(load_library().grx_graph_copy_to_host(self._h, ap.ctypes.data, aj.ctypes.data,
                                                     ax.ctypes.data), "grx_graph_copy_to_host")
        return ap, aj[: self.nnz], ax[: self.nnz]

    def offsets_to_host(self):
        """Row offsets only (4 (V + 1) bytes; to_host() moves 8 bytes per edge as well)."""
        ap = np.empty(self.n_rows + 1, np.int32)
        _check(load_library().grx_graph_copy_to_host(self._h, ap.ctypes.data, None, None),
               "grx_graph_copy_to_host")
        return ap

    def close(self) -> None:
        if self._h:
            load_library().grx_graph_destroy(self._h)
            self._h = _VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _torch():
    import torch
    return torch


def bfs(ctx: Context, g: Graph, source: int, distances=None, options: Optional[Options] = None):
    """gunrock::bfs::run -> (int32 depths on the device, Stats)."""
    torch = _torch()
    if distances is None:
        distances = torch.empty(g.n_rows, dtype=torch.int32, device=f"cuda:{ctx.device}")
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_bfs(ctx._h, g._h, source, _ptr(distances), None, C.byref(o),
                                  C.byref(s)), "grx_bfs")
    return distances, Stats._from(s)


def sssp(ctx: Context, g: Graph, source: int, distances=None, options: Optional[Options] = None):
    """gunrock::sssp::run -> (float32 distances on the device, Stats)."""
    torch = _torch()
    if distances is None:
        distances = torch.empty(g.n_rows, dtype=torch.float32, device=f"cuda:{ctx.device}")
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_sssp(ctx._h, g._h, source, _ptr(distances), None, C.byref(o),
                                   C.byref(s)), "grx_sssp")
    return distances, Stats._from(s)


def pagerank(ctx: Context, g: Graph, alpha: float = 0.85, tol: float = 1e-6, p=None,
             options: Optional[Options] = None):
    """gunrock::pr::run -> (float32 ranks on the device, Stats)."""
    torch = _torch()
    if p is None:
        p = torch.empty(g.n_rows, dtype=torch.float32, device=f"cuda:{ctx.device}")
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_pagerank(ctx._h, g._h, alpha, tol, _ptr(p), C.byref(o), C.byref(s)),
           "grx_pagerank")
    return p, Stats._from(s)


def bc(ctx: Context, g: Graph, sources=None, bc_values=None, options: Optional[Options] = None):
    """gunrock::bc::run summed over `sources` -> (float32 centralities on the device, Stats).

    `sources`: None (every vertex), one vertex, or a sequence / numpy array of vertices;
    bc[v] = 0.5 * sum over the sources s of Brandes' dependency delta_s(v)."""
    torch = _torch()
    if bc_values is None:
        bc_values = torch.empty(g.n_rows, dtype=torch.float32, device=f"cuda:{ctx.device}")
    if sources is None:
        h, n = None, 0
    else:
        h = np.ascontiguousarray(np.atleast_1d(np.asarray(sources)), dtype=np.int32)
        if h.ndim != 1:
            raise ValueError("bc: sources must be one vertex or a flat list of vertices")
        n = int(h.size)
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_bc(ctx._h, g._h, _ptr(h) if h is not None else None, n, _ptr(bc_values),
                                 C.byref(o), C.byref(s)), "grx_bc")
    return bc_values, Stats._from(s)


def tc(ctx: Context, g: Graph, counts=None, per_vertex: bool = True, options: Optional[Options] = None):
    """gunrock::tc::run on the simple undirected graph under a symmetric CSR -> (int64 per-vertex
    triangle counts on the device or None, distinct triangles T as an int, Stats).

    `counts`: int64 tensor of V on the context's device, allocated when None; per_vertex=False
    computes T only (counts is then None).  Self loops and repeated entries are ignored, row order
    does not matter; the sum of the per-vertex counts is 3 * T."""
    torch = _torch()
    if not per_vertex:
        counts = None
    elif counts is None:
        counts = torch.empty(g.n_rows, dtype=torch.int64, device=f"cuda:{ctx.device}")
    total = C.c_uint64()
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_tc(ctx._h, g._h, _ptr(counts), C.byref(total), C.byref(o), C.byref(s)),
           "grx_tc")
    return counts, int(total.value), Stats._from(s)


def _vertex_output(ctx: Context, g: Graph, t, call: str, what: str):
    """The int32 output tensor `what` of `call`: allocated when None, else checked to be a contiguous
    tensor of V on the context's device."""
    torch = _torch()
    device = torch.device(f"cuda:{ctx.device}")
    if t is None:
        return torch.empty(g.n_rows, dtype=torch.int32, device=device)
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise TypeError(f"{call}: {what} must be an int32 torch tensor")
    if t.dim() != 1 or t.numel() != g.n_rows or not t.is_contiguous():
        raise ValueError(f"{call}: {what} must be a contiguous tensor of {g.n_rows} elements")
    if t.device != device:
        raise ValueError(f"{call}: {what} must live on {device}")
    return t


def kcore(ctx: Context, g: Graph, cores=None, options: Optional[Options] = None):
    """gunrock::kcore::run on a symmetric CSR -> (int32 core numbers on the device, degeneracy as an
    int, Stats).

    `cores`: int32 tensor of V on the context's device, allocated when None.  Every entry of the CSR
    counts (repeats each time, a self loop once): `g.simple(ctx)` gives the textbook core numbers
    of the simple graph under a multigraph.  Stats.iterations is the number of distinct non-zero
    core values and Stats.edges_expanded equals nnz (every row is walked once)."""
    torch = _torch()
    if cores is None:
        cores = torch.empty(g.n_rows, dtype=torch.int32, device=f"cuda:{ctx.device}")
    degeneracy = C.c_int32()
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_kcore(ctx._h, g._h, _ptr(cores), C.byref(degeneracy), C.byref(o), C.byref(s)),
           "grx_kcore")
    return cores, int(degeneracy.value), Stats._from(s)


def color(ctx: Context, g: Graph, colors=None, options: Optional[Options] = None):
    """Greedy colouring of a symmetric CSR in largest-degree-first order -> (int32 colours on the
    device, number of colours as an int, Stats).

    colors[v] is the smallest colour >= 0 that no neighbour of larger key has, with key(v) =
    (row length << 32) | fmix32(v) (include/essentials_amd.h): a function of the CSR alone, the
    same on every call, and adjacent vertices never share a colour.  `colors`: int32 contiguous
    tensor of V on the context's device, allocated when None and filled in place otherwise.
    Stats.iterations is the depth of the priority DAG and Stats.edges_expanded equals 2 * nnz."""
    colors = _vertex_output(ctx, g, colors, "color", "colors")
    count = C.c_int32()
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_color(ctx._h, g._h, _ptr(colors), C.byref(count), C.byref(o), C.byref(s)),
           "grx_color")
    return colors, int(count.value), Stats._from(s)


def cc(ctx: Context, g: Graph, components=None, options: Optional[Options] = None):
    """Connected components (weakly connected on a directed CSR) -> (int32 labels on the device,
    number of components as an int, Stats).

    labels[v] is the smallest vertex id of the component that holds v, so labels[v] == v marks a
    component's representative and `torch.bincount(labels)` gives the component sizes.
    `components`: int32 contiguous tensor of V on the context's device, allocated when None.
    Stats.vertices_reached is V - components; Stats.edges_expanded counts the row entries read, nnz
    unless the graph is known to be symmetric, when the rows of the largest component stay unread."""
    components = _vertex_output(ctx, g, components, "cc", "components")
    count = C.c_int64()
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_cc(ctx._h, g._h, _ptr(components), C.byref(count), C.byref(o), C.byref(s)),
           "grx_cc")
    return components, int(count.value), Stats._from(s)


def scc(ctx: Context, g: Graph, components=None, options: Optional[Options] = None):
    """Strongly connected components -> (int32 labels on the device, number of components as an int,
    Stats).

    labels[v] is the smallest vertex id of the strongly connected component that holds v, the
    convention of `cc`: labels[v] == v marks a representative, a vertex on no cycle is a component of
    one.  A directed graph needs its in-edges (`g.build_in_edges(ctx)`); without them a symmetric CSR
    is answered by `cc` and an asymmetric one raises EngineError.  `components`: int32 contiguous
    tensor of V on the context's device, allocated when None and filled in place otherwise.
    Stats.iterations is the number of forward-backward rounds (0 when trimming finished everything),
    Stats.vertices_reached is V - components and Stats.edges_expanded the row entries of either
    array read."""
    components = _vertex_output(ctx, g, components, "scc", "components")
    count = C.c_int64()
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_scc(ctx._h, g._h, _ptr(components), C.byref(count), C.byref(o), C.byref(s)),
           "grx_scc")
    return components, int(count.value), Stats._from(s)


def lpa(ctx: Context, g: Graph, communities=None, options: Optional[Options] = None):
    """Communities of a symmetric CSR by semi-synchronous label propagation over the colour classes
    of `color` -> (int32 labels on the device, number of communities as an int, modularity as a
    float, Stats).

    labels[v] is the smallest vertex id of the community that holds v, the convention of `cc`.  A
    sweep lets every vertex of one colour class at a time take the most frequent label among its
    neighbours (repeats count, self loops do not; it keeps its own when that is among the most
    frequent, else the one of smallest fmix32: include/essentials_amd.h), and the call stops after
    the first sweep that changes nothing or after Options.max_iterations sweeps: a function of the
    CSR alone, the same on every call.  `communities`: int32 contiguous tensor of V on the context's
    device, allocated when None and filled in place otherwise.  The modularity is `modularity` of the
    result.  Stats.iterations is the number of sweeps, Stats.frontier_slots the labels changed per
    sweep and Stats.vertices_reached V - communities."""
    communities = _vertex_output(ctx, g, communities, "lpa", "communities")
    count = C.c_int64()
    q = C.c_double()
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_lpa(ctx._h, g._h, _ptr(communities), C.byref(count), C.byref(q), C.byref(o),
                                  C.byref(s)), "grx_lpa")
    return communities, int(count.value), float(q.value), Stats._from(s)


def louvain(ctx: Context, g: Graph, communities=None, options: Optional[Options] = None):
    """Communities of a symmetric CSR by multi-level modularity optimisation (Louvain) in exact
    integers -> (int32 labels on the device, number of communities as an int, modularity as a
    float, levels as an int, Stats).

    labels[v] is the smallest vertex id of the community that holds v, the convention of `cc` and
    `lpa`.  A phase sweeps the colour classes of `color` on its level graph: every vertex of a class
    moves to the neighbouring community of largest integer gain k_vc * E - k(v) * tot(c) (smallest
    fmix32 among equals) when that beats staying; a sweep that does not raise the score is undone
    and ends the phase, and the communities become the next level's vertices
    (include/essentials_amd.h states all of it).  A function of the CSR alone, the same bits on
    every call.  Options.max_iterations, when not 0, is the number of phases: the result is then a
    cut of the dendrogram.  Resolution is fixed at 1.  `communities`: int32 contiguous tensor of V
    on the context's device, allocated when None and filled in place otherwise.  The modularity is
    `modularity` of the result.  `levels` counts the phases run, the last one, which keeps nothing,
    included.  Stats.iterations is the number of sweeps over all phases, Stats.frontier_slots the
    moves each kept (0 ends a phase) and Stats.vertices_reached V - communities."""
    communities = _vertex_output(ctx, g, communities, "louvain", "communities")
    count = C.c_int64()
    q = C.c_double()
    levels = C.c_int32()
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_louvain(ctx._h, g._h, _ptr(communities), C.byref(count), C.byref(q), C.byref(levels),
                                      C.byref(o), C.byref(s)), "grx_louvain")
    return communities, int(count.value), float(q.value), int(levels.value), Stats._from(s)


def modularity(ctx: Context, g: Graph, labels):
    """Modularity of a labelling in exact integers -> (Q as a float, I = the entries whose ends share
    a label, S = the sum over labels of (the row lengths of its vertices) squared), with E = nnz and
    Q = I / E - S / E^2 (0.0 when E == 0).

    `labels`: int32 contiguous tensor of V on the context's device with values in [0, V), such as
    the result of `lpa`, `cc` or `scc`; a value outside raises EngineError.  Every entry counts as
    given, self loops and repeats included; on a simple symmetric graph this is
    networkx.community.modularity at resolution 1."""
    if labels is None:
        raise TypeError("modularity: labels must be an int32 torch tensor")
    labels = _vertex_output(ctx, g, labels, "modularity", "labels")
    q = C.c_double()
    inside = C.c_int64()
    squares = C.c_uint64()
    ctx.after_torch()
    _check(load_library().grx_modularity(ctx._h, g._h, _ptr(labels), C.byref(q), C.byref(inside), C.byref(squares),
                                         None, None), "grx_modularity")
    return float(q.value), int(inside.value), int(squares.value)


def mst(ctx: Context, g: Graph, entries=None, components=None, options: Optional[Options] = None):
    """Minimum spanning forest of the CSR as given -> (int32 chosen entry positions on the device,
    ascending; their total weight as a float; int32 component labels or None; Stats).

    Every row entry is an undirected candidate, ordered by (weight, position): the result is what
    Kruskal accepts in that order (include/essentials_amd.h).  The returned `entries` is the tensor
    sliced to the count, V - components; position e is an index into the column and value arrays.
    `entries`: int32 contiguous tensor of V on the context's device, allocated when None and filled
    in place otherwise.  `components`: None (no labels), True (allocate them) or such a tensor of
    V; the labels are those of `cc`.  Stats.iterations is the number of Boruvka rounds and
    Stats.edges_expanded the row entries the minimum search read, summed over rounds."""
    entries = _vertex_output(ctx, g, entries, "mst", "entries")
    if components is False:
        components = None
    elif components is not None:
        components = _vertex_output(ctx, g, None if components is True else components, "mst", "components")
    count, weight = C.c_int64(), C.c_double()
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_mst(ctx._h, g._h, _ptr(entries), C.byref(count), C.byref(weight),
                                  _ptr(components), C.byref(o), C.byref(s)), "grx_mst")
    return entries[: count.value], float(weight.value), components, Stats._from(s)


def spgemm(ctx: Context, a: Graph, b: Graph, options: Optional[Options] = None):
    """Sparse matrix product C = A * B -> (Graph, Stats): a new owning graph of a.n_rows x b.n_cols.

    C has an entry (i, j) iff some entry (i, k) of A meets an entry (k, j) of B; each is stored once,
    rows sorted by column, and an entry whose products cancel stays with value 0.0.  Values are
    float32 sums in an order the call does not promise: exact and the same on every call when the
    partial sums are representable (integer weights, sum |products| < 2**24 per entry), within the
    summation bound of the float64 sum otherwise (include/essentials_amd.h).  `a is b` is allowed.
    More than 2**31 - 1 entries raise EngineError (-3).  Stats.edges_expanded is the number of
    products, Stats.edges_traversed nnz(C), Stats.vertices_reached the rows of C with an entry; with
    collect_kernel_time Stats.frontier_slots holds the microseconds of the bound, symbolic and
    numeric batches."""
    h = _VP()
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_spgemm(ctx._h, a._h, b._h, C.byref(h), C.byref(o), C.byref(s)), "grx_spgemm")
    return Graph(h), Stats._from(s)


def truss(ctx: Context, g: Graph, values=None, options: Optional[Options] = None):
    """K-truss decomposition of the simple undirected graph under a symmetric CSR -> (int32 trussness
    per CSR entry on the device, the largest trussness as an int, Stats).

    values[p] is the largest k >= 2 such that the edge entry p names lies in the k-truss, the maximal
    subgraph whose every edge is in at least k - 2 of its triangles (the convention of
    networkx.k_truss: an edge in no triangle has 2, every edge of K_n has n).  The k-truss subgraph
    is `values >= k`.  Self loops and repeated entries are ignored and row order does not matter:
    both directions and every repeat of an edge carry the same value, a self loop carries 0.
    `values`: int32 contiguous tensor of g.nnz on the context's device, allocated when None and
    filled in place otherwise.  The same call returns identical values.  Stats.iterations is the
    number of distinct values of the answer, Stats.edges_traversed the number m of distinct
    undirected edges and Stats.edges_expanded the row entries the intersections read; with
    collect_kernel_time Stats.frontier_slots holds the microseconds of the copy, support and peel
    phases."""
    torch = _torch()
    device = torch.device(f"cuda:{ctx.device}")
    if values is None:
        values = torch.empty(g.nnz, dtype=torch.int32, device=device)
    else:
        if not isinstance(values, torch.Tensor) or values.dtype != torch.int32:
            raise TypeError("truss: values must be an int32 torch tensor")
        if values.dim() != 1 or values.numel() != g.nnz or not values.is_contiguous():
            raise ValueError(f"truss: values must be a contiguous tensor of {g.nnz} elements")
        if values.device != device:
            raise ValueError(f"truss: values must live on {device}")
    largest = C.c_int32()
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_truss(ctx._h, g._h, _ptr(values), C.byref(largest), C.byref(o), C.byref(s)),
           "grx_truss")
    return values, int(largest.value), Stats._from(s)


def bfs_multi(ctx: Context, g: Graph, sources=None, depths=None, want_depths: bool = True,
              options: Optional[Options] = None):
    """Multi-source BFS, 64 searches to a 64-bit word per vertex -> (int32 depths [count, V] on the
    device or None, summary, Stats).

    `sources`: None (every vertex), one vertex, or a sequence / numpy array of vertices, as for `bc`;
    a vertex named twice is searched twice.  Row i of the depths is what `bfs` gives from source i
    (INT_UNREACHED where unreached).  `depths`: int32 contiguous tensor of count * V elements on the
    context's device, allocated when None; want_depths=False computes the summaries only (no
    count * V array exists then) and returns None for the depths.  `summary` is a dict of numpy
    arrays of count: `reached` (int64, vertices with a finite depth, the source included),
    `depth_sum` (int64, the sum of the finite depths) and `eccentricity` (int32, the largest one);
    closeness of source i is (reached[i] - 1) / depth_sum[i].  Options read: collect_kernel_time,
    direction_optimized and do_alpha.  Stats.iterations is the sum over batches of 64 of 1 + the
    largest eccentricity in the batch, Stats.edges_traversed the out-degrees of every level's
    active vertices (the work a batch shares) and Stats.frontier_slots the first batch's levels."""
    torch = _torch()
    device = torch.device(f"cuda:{ctx.device}")
    if sources is None:
        h, n, count = None, 0, g.n_rows
    else:
        h = np.ascontiguousarray(np.atleast_1d(np.asarray(sources)), dtype=np.int32)
        if h.ndim != 1:
            raise ValueError("bfs_multi: sources must be one vertex or a flat list of vertices")
        n = count = int(h.size)
        if n == 0:  # an empty list is not "every vertex": hand the ABI a non-NULL pointer
            h = np.zeros(1, np.int32)
    if not want_depths:
        depths = None
    elif depths is None:
        depths = torch.empty((count, g.n_rows), dtype=torch.int32, device=device)
    else:
        if not isinstance(depths, torch.Tensor) or depths.dtype != torch.int32:
            raise TypeError("bfs_multi: depths must be an int32 torch tensor")
        if depths.numel() != count * g.n_rows or not depths.is_contiguous():
            raise ValueError(f"bfs_multi: depths must be a contiguous tensor of {count} x {g.n_rows} elements")
        if depths.device != device:
            raise ValueError(f"bfs_multi: depths must live on {device}")
        depths = depths.view(count, g.n_rows)
    # the host arrays are never NULL, so an empty depths tensor (a NULL pointer) is no argument error
    reached = np.zeros(max(count, 1), np.int64)
    depth_sum = np.zeros(max(count, 1), np.int64)
    eccentricity = np.zeros(max(count, 1), np.int32)
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_bfs_multi(ctx._h, g._h, _ptr(h), n,
                                        _ptr(depths) if depths is not None and depths.numel() else None,
                                        _ptr(reached), _ptr(depth_sum), _ptr(eccentricity), C.byref(o), C.byref(s)),
           "grx_bfs_multi")
    summary = {"reached": reached[:count], "depth_sum": depth_sum[:count], "eccentricity": eccentricity[:count]}
    return depths, summary, Stats._from(s)


def ppr(ctx: Context, g: Graph, seeds=None, alpha: float = 0.85, tol: float = 1e-6, p=None,
        options: Optional[Options] = None):
    """Batched personalized PageRank, 64 seeds to a wavefront -> (float32 ranks [count, V] on the
    device, info, Stats).

    `seeds`: None (every vertex), one vertex, or a sequence / numpy array of vertices, as for
    `bfs_multi`; a vertex named twice is a row of its own.  Row i is the PageRank vector restarted at
    seed i: the power iteration of `pagerank` with the teleport and the dangling mass returned to the
    seed (networkx.pagerank(personalization={s: 1})), so each row sums to 1.  A row stops after the
    first iteration whose largest change is below `tol`, or after Options.max_iterations when that is
    non-zero (tol <= 0 needs it), and is frozen from then on: it is bit-identical to the single-seed
    call whatever else is in the list, and the same call returns identical values
    (include/essentials_amd.h).  A directed graph needs its in-edges (`g.build_in_edges(ctx)`); an
    asymmetric CSR without them raises EngineError.  `p`: float32 contiguous tensor of count * V
    elements on the context's device, allocated when None.  `info` is a dict of numpy arrays of
    count: `iterations` (int32) and `residual` (float32, the last largest change).  Options read:
    collect_kernel_time and max_iterations.  Stats.iterations is the sum over batches of 64 of the
    batch's largest iteration count, Stats.vertices_reached the entries > 0 and Stats.frontier_slots
    the unfrozen rows of the first batch per iteration."""
    torch = _torch()
    device = torch.device(f"cuda:{ctx.device}")
    if seeds is None:
        h, n, count = None, 0, g.n_rows
    else:
        h = np.ascontiguousarray(np.atleast_1d(np.asarray(seeds)), dtype=np.int32)
        if h.ndim != 1:
            raise ValueError("ppr: seeds must be one vertex or a flat list of vertices")
        n = count = int(h.size)
        if n == 0:  # an empty list is not "every vertex": hand the ABI a non-NULL pointer
            h = np.zeros(1, np.int32)
    if p is None:
        p = torch.empty((count, g.n_rows), dtype=torch.float32, device=device)
    else:
        if not isinstance(p, torch.Tensor) or p.dtype != torch.float32:
            raise TypeError("ppr: p must be a float32 torch tensor")
        if p.numel() != count * g.n_rows or not p.is_contiguous():
            raise ValueError(f"ppr: p must be a contiguous tensor of {count} x {g.n_rows} elements")
        if p.device != device:
            raise ValueError(f"ppr: p must live on {device}")
        p = p.view(count, g.n_rows)
    iterations = np.zeros(max(count, 1), np.int32)
    residual = np.zeros(max(count, 1), np.float32)
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_ppr(ctx._h, g._h, _ptr(h), n, alpha, tol, _ptr(p) if p.numel() else None,
                                  _ptr(iterations), _ptr(residual), C.byref(o), C.byref(s)), "grx_ppr")
    return p, {"iterations": iterations[:count], "residual": residual[:count]}, Stats._from(s)


def _float_vector(ctx: Context, t, length: int, call: str, what: str):
    """The float32 tensor `what` of `call`: allocated when None, else checked to be a contiguous
    tensor of `length` on the context's device."""
    torch = _torch()
    device = torch.device(f"cuda:{ctx.device}")
    if t is None:
        return torch.empty(length, dtype=torch.float32, device=device)
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"{call}: {what} must be a float32 torch tensor")
    if t.dim() != 1 or t.numel() != length or not t.is_contiguous():
        raise ValueError(f"{call}: {what} must be a contiguous tensor of {length} elements")
    if t.device != device:
        raise ValueError(f"{call}: {what} must live on {device}")
    return t


def spmv(ctx: Context, g: Graph, x, transpose: bool = False, y=None, options: Optional[Options] = None):
    """y = A x over the graph's entries, or y = A^T x -> (float32 y on the device, Stats).

    `x`: float32 contiguous tensor on the context's device, of n_cols elements (n_rows when
    transposed); `y`: the same of n_rows (n_cols), allocated when None, overwritten in full; the two
    must not overlap.  Every row sum has a fixed order: the same call returns identical bits, and the
    exact value whenever float32 holds every partial sum (include/essentials_amd.h).  The transposed
    product is a pull over in-rows: a directed graph needs its in-edges (`g.build_in_edges(ctx)`), an
    asymmetric CSR without them and a rectangular graph raise EngineError.  The engine's stream waits
    for what torch has enqueued, so `x` may come straight from torch work.  Options read:
    collect_kernel_time."""
    if x is None:
        raise TypeError("spmv: x must be a float32 torch tensor")
    x = _float_vector(ctx, x, g.n_rows if transpose else g.n_cols, "spmv", "x")
    y = _float_vector(ctx, y, g.n_cols if transpose else g.n_rows, "spmv", "y")
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_spmv(ctx._h, g._h, int(bool(transpose)), _ptr(x) if x.numel() else None,
                                   _ptr(y) if y.numel() else None, C.byref(o), C.byref(s)), "grx_spmv")
    return y, Stats._from(s)


def _float_matrix(ctx: Context, t, rows: int, features: Optional[int], call: str, what: str):
    """The float32 matrix `what` of `call` -> (tensor, its leading dimension in elements): allocated
    contiguous when None, else checked to be a 2-D tensor of `rows` rows (and `features` columns when
    given) on the context's device whose rows are contiguous and do not run into each other."""
    torch = _torch()
    device = torch.device(f"cuda:{ctx.device}")
    if t is None:
        t = torch.empty((rows, features), dtype=torch.float32, device=device)
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"{call}: {what} must be a float32 torch tensor")
    if t.dim() != 2 or t.shape[0] != rows or (features is not None and t.shape[1] != features):
        shape = f"{rows} x {'F' if features is None else features}"
        raise ValueError(f"{call}: {what} must be a 2-D tensor of {shape} elements")
    F = t.shape[1]
    # a stride of a dimension of one element (or none) addresses nothing
    if (F > 1 and t.stride(1) != 1) or (rows > 1 and t.stride(0) < F):
        raise ValueError(f"{call}: {what} must have stride(1) == 1 and stride(0) >= {F}")
    if t.device != device:
        raise ValueError(f"{call}: {what} must live on {device}")
    return t, (max(t.stride(0), F) if rows > 1 else F)


def spmm(ctx: Context, g: Graph, x, transpose: bool = False, y=None, options: Optional[Options] = None,
         values=None):
    """Y = A X over the graph's entries for a dense feature matrix, or Y = A^T X -> (float32 Y on
    the device, Stats).

    `x`: float32 2-D tensor on the context's device of n_cols rows (n_rows when transposed) and F
    columns with stride(1) == 1 and stride(0) >= F: row-strided views are accepted as they are.  `y`:
    the same of n_rows (n_cols) rows and F columns, allocated contiguous when None; its columns
    [0, F) are overwritten, what lies between its rows is neither read nor written; the two must not
    overlap.  Every element is summed over its row's entries in row order, rows above
    GRX_SPMM_SEGMENT = 512 entries in segments whose sums are added in order: the same call returns
    identical bits, column f is bit for bit the F = 1 call on that column, and the value is exact
    whenever float32 holds every partial sum (include/essentials_amd.h).  The transposed product is a
    pull over in-rows under `spmv`'s rule: a directed graph needs its in-edges
    (`g.build_in_edges(ctx)`), an asymmetric CSR without them and a rectangular graph raise
    EngineError.  The engine's stream waits for what torch has enqueued.  Options read:
    collect_kernel_time.

    `values`: None multiplies by the values the graph was built with (grx_spmm).  Otherwise a
    contiguous float32 tensor of nnz elements on the context's device, in the order of the CSR's
    entries, takes their place (grx_spmm_values); it must not overlap `y`, and the result has the bits
    of `spmm` on a graph built from the same structure with those values.  With `values` the
    transposed product needs the in-edges on every graph, a symmetric one included."""
    if x is None:
        raise TypeError("spmm: x must be a float32 torch tensor")
    if values is not None:
        values = _float_vector(ctx, values, g.nnz, "spmm", "values")
    x, ldx = _float_matrix(ctx, x, g.n_rows if transpose else g.n_cols, None, "spmm", "x")
    F = x.shape[1]
    y, ldy = _float_matrix(ctx, y, g.n_cols if transpose else g.n_rows, F, "spmm", "y")
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    px, py = _ptr(x) if x.numel() else None, _ptr(y) if y.numel() else None
    if values is None:
        _check(load_library().grx_spmm(ctx._h, g._h, int(bool(transpose)), F, px, ldx, py, ldy, C.byref(o),
                                       C.byref(s)), "grx_spmm")
    else:
        _check(load_library().grx_spmm_values(ctx._h, g._h, _ptr(values) if values.numel() else None,
                                              int(bool(transpose)), F, px, ldx, py, ldy, C.byref(o), C.byref(s)),
               "grx_spmm_values")
    return y, Stats._from(s)


def sddmm(ctx: Context, g: Graph, u, v, out=None, options: Optional[Options] = None):
    """out[e] = <u[row(e)], v[col(e)]> for every entry e of the graph's CSR, at the entry's position in
    the column array -> (float32 out of nnz elements on the device, Stats).

    `u`: float32 2-D tensor on the context's device of n_rows rows and F columns, `v`: of n_cols rows
    and F columns, both with stride(1) == 1 and stride(0) >= F (row-strided views are accepted as they
    are); they may be the same tensor.  `out`: contiguous float32 of nnz elements, allocated when None,
    overwritten in full; it must not overlap `u` or `v`.  The graph's values are not read.  Every dot
    product is summed in an order that depends on F alone (include/essentials_amd.h): the same call
    returns identical bits, and the exact value whenever float32 holds every partial sum.  The engine's
    stream waits for what torch has enqueued.  Options read: collect_kernel_time."""
    if u is None or v is None:
        raise TypeError("sddmm: u and v must be float32 torch tensors")
    u, ldu = _float_matrix(ctx, u, g.n_rows, None, "sddmm", "u")
    F = u.shape[1]
    v, ldv = _float_matrix(ctx, v, g.n_cols, F, "sddmm", "v")
    out = _float_vector(ctx, out, g.nnz, "sddmm", "out")
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_sddmm(ctx._h, g._h, F, _ptr(u) if u.numel() else None, ldu,
                                    _ptr(v) if v.numel() else None, ldv, _ptr(out) if out.numel() else None,
                                    C.byref(o), C.byref(s)), "grx_sddmm")
    return out, Stats._from(s)


def spmm_autograd(ctx: Context, g: Graph, x, values=None):
    """`spmm(ctx, g, x, values=values)[0]` as a differentiable function: the backward pass is the
    transposed product of the incoming gradient, so it raises at backward time whatever
    `spmm(..., transpose=True)` raises on this graph.  Without `values` the graph's values are
    constants and `x` is the one input.  With `values` (the per-entry values of `spmm`) the function is
    differentiable in both: grad_x = spmm(grad, values=values, transpose=True), which needs the
    in-edges, and grad_values = sddmm(grad, x); each is computed only where a gradient is asked for."""
    torch = _torch()

    if values is None:
        class _Product(torch.autograd.Function):
            @staticmethod
            def forward(fctx, features):
                return spmm(ctx, g, features)[0]

            @staticmethod
            def backward(fctx, grad):
                return spmm(ctx, g, grad.contiguous(), transpose=True)[0]

        return _Product.apply(x)

    class _WeightedProduct(torch.autograd.Function):
        @staticmethod
        def forward(fctx, features, w):
            fctx.save_for_backward(features, w)
            return spmm(ctx, g, features, values=w)[0]

        @staticmethod
        def backward(fctx, grad):
            features, w = fctx.saved_tensors
            grad = grad.contiguous()
            grad_x = grad_w = None
            if fctx.needs_input_grad[0]:
                grad_x = spmm(ctx, g, grad, values=w, transpose=True)[0]
            if fctx.needs_input_grad[1]:
                grad_w = sddmm(ctx, g, grad, features)[0]
            return grad_x, grad_w

    return _WeightedProduct.apply(x, values)


def sddmm_autograd(ctx: Context, g: Graph, u, v):
    """`sddmm(ctx, g, u, v)[0]` as a differentiable function of `u` and `v`: grad_u =
    spmm(v, values=grad) and grad_v = spmm(u, values=grad, transpose=True), each computed only where a
    gradient is asked for.  The backward pass raises whatever those calls raise: grad_v needs the
    graph's in-edges (`g.build_in_edges(ctx)`) and a square graph."""
    torch = _torch()

    class _Scores(torch.autograd.Function):
        @staticmethod
        def forward(fctx, left, right):
            fctx.save_for_backward(left, right)
            return sddmm(ctx, g, left, right)[0]

        @staticmethod
        def backward(fctx, grad):
            left, right = fctx.saved_tensors
            grad = grad.contiguous()
            grad_u = grad_v = None
            if fctx.needs_input_grad[0]:
                grad_u = spmm(ctx, g, right, values=grad)[0]
            if fctx.needs_input_grad[1]:
                grad_v = spmm(ctx, g, left, values=grad, transpose=True)[0]
            return grad_u, grad_v

    return _Scores.apply(u, v)


def _by_column(call: str, by) -> int:
    if by not in ("row", "column"):
        raise ValueError(f"{call}: by must be \"row\" or \"column\", not {by!r}")
    return int(by == "column")


def edge_softmax(ctx: Context, g: Graph, scores, by: str = "row", out=None, options: Optional[Options] = None):
    """out[e] = exp(scores[e] - m) / sum of exp(scores[e'] - m) over the entries e' that share e's row
    (`by="row"`) or column (`by="column"`), m their largest score -> (float32 out of nnz elements on the
    device, Stats): the attention coefficients of the scores that `sddmm` returns, in the order `spmm`
    takes as `values`.

    `scores`: contiguous float32 tensor of nnz elements on the context's device, in the order of the
    CSR's entries; `out`: the same, allocated when None, overwritten in full; the two must not overlap.
    The graph's values and column ids are not read.  Every sum has a fixed order
    (include/essentials_amd.h): the same call returns identical bits, and a group's results are those
    of a graph that holds nothing but that group.  A group with a NaN or +inf score is NaN throughout,
    as `torch.softmax` gives; a group whose scores are all -inf gets zeros; an empty group writes
    nothing.  `by="column"` needs the graph's in-edges (`g.build_in_edges(ctx)`) on every graph, a
    symmetric one included, and a square graph; EngineError otherwise.  The engine's stream waits for
    what torch has enqueued.  Options read: collect_kernel_time."""
    column = _by_column("edge_softmax", by)
    if scores is None:
        raise TypeError("edge_softmax: scores must be a float32 torch tensor")
    scores = _float_vector(ctx, scores, g.nnz, "edge_softmax", "scores")
    out = _float_vector(ctx, out, g.nnz, "edge_softmax", "out")
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_edge_softmax(ctx._h, g._h, column, _ptr(scores) if scores.numel() else None,
                                           _ptr(out) if out.numel() else None, C.byref(o), C.byref(s)),
           "grx_edge_softmax")
    return out, Stats._from(s)


def edge_softmax_backward(ctx: Context, g: Graph, probabilities, grad, by: str = "row", out=None,
                          options: Optional[Options] = None):
    """out[e] = probabilities[e] * (grad[e] - D), D the sum of probabilities[e'] * grad[e'] over the
    entries e' of e's group -> (float32 out of nnz elements on the device, Stats): the gradient with
    respect to the scores of `edge_softmax`, given its output and the gradient with respect to that.

    The three vectors are contiguous float32 tensors of nnz elements on the context's device in the
    order of the CSR's entries; `out` is allocated when None and must not overlap an input, the inputs
    may be one tensor.  `probabilities` need not be a softmax result.  D is summed in `edge_softmax`'s
    order, one fused multiply-add per entry; the same call returns identical bits.  `by` as for
    `edge_softmax`.  Options read: collect_kernel_time."""
    column = _by_column("edge_softmax_backward", by)
    if probabilities is None or grad is None:
        raise TypeError("edge_softmax_backward: probabilities and grad must be float32 torch tensors")
    probabilities = _float_vector(ctx, probabilities, g.nnz, "edge_softmax_backward", "probabilities")
    grad = _float_vector(ctx, grad, g.nnz, "edge_softmax_backward", "grad")
    out = _float_vector(ctx, out, g.nnz, "edge_softmax_backward", "out")
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    none = out.numel() == 0
    _check(load_library().grx_edge_softmax_backward(ctx._h, g._h, column, None if none else _ptr(probabilities),
                                                    None if none else _ptr(grad), None if none else _ptr(out),
                                                    C.byref(o), C.byref(s)), "grx_edge_softmax_backward")
    return out, Stats._from(s)


def edge_softmax_autograd(ctx: Context, g: Graph, scores, by: str = "row"):
    """`edge_softmax(ctx, g, scores, by)[0]` as a differentiable function of `scores`: the output is
    saved and the backward pass is `edge_softmax_backward(out, grad)`.  It raises at forward time
    whatever `edge_softmax` raises."""
    torch = _torch()

    class _Coefficients(torch.autograd.Function):
        @staticmethod
        def forward(fctx, s):
            out = edge_softmax(ctx, g, s, by)[0]
            fctx.save_for_backward(out)
            return out

        @staticmethod
        def backward(fctx, grad):
            (out,) = fctx.saved_tensors
            return edge_softmax_backward(ctx, g, out, grad.contiguous(), by)[0]

    return _Coefficients.apply(scores)


def hits(ctx: Context, g: Graph, tol: float = 1e-6, hubs=None, authorities=None, normalized: bool = False,
         options: Optional[Options] = None):
    """HITS hub and authority scores -> (float32 hubs, float32 authorities on the device, info, Stats).

    Power iteration from h = 1: authorities = in-rows times hubs, hubs = out-rows times authorities,
    each divided by its largest magnitude; the run stops after the first iteration whose largest hub
    change is below `tol`, or after Options.max_iterations when that is non-zero (tol <= 0 needs it).
    Weights are read as they are.  Every sum has a fixed order: the same call returns identical bits
    (include/essentials_amd.h).  A directed graph needs its in-edges (`g.build_in_edges(ctx)`); an
    asymmetric CSR without them raises EngineError.  `hubs`, `authorities`: float32 contiguous
    tensors of V on the context's device, allocated when None.  `info` = {"iterations": int,
    "residual": float} (the last largest change).  normalized=False delivers the engine's values
    untouched (largest entry 1); normalized=True divides each vector by its float64 sum, networkx's
    convention (a vector that sums to 0 is left as it is).  Options read: collect_kernel_time and
    max_iterations.  Stats.edges_traversed is 2 * nnz * iterations and Stats.vertices_reached the
    vertices with a hub or authority value > 0."""
    torch = _torch()
    hubs = _float_vector(ctx, hubs, g.n_rows, "hits", "hubs")
    authorities = _float_vector(ctx, authorities, g.n_rows, "hits", "authorities")
    iterations = C.c_int32()
    residual = C.c_float()
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_hits(ctx._h, g._h, tol, _ptr(hubs) if hubs.numel() else None,
                                   _ptr(authorities) if authorities.numel() else None, C.byref(iterations),
                                   C.byref(residual), C.byref(o), C.byref(s)), "grx_hits")
    if normalized:
        for v in (hubs, authorities):
            total = float(v.sum(dtype=torch.float64)) if v.numel() else 0.0
            if total != 0.0:
                v.copy_((v.double() / total).float())
    return hubs, authorities, {"iterations": int(iterations.value), "residual": float(residual.value)}, Stats._from(s)


def predecessors(ctx: Context, g: Graph, source: int, labels, predecessors=None, hops: bool = False,
                 options: Optional[Options] = None):
    """The shortest-path tree that finished labels imply -> (int32 predecessors on the device, int32
    hops on the device or None, {"orphans": int, "violations": int}, Stats).

    `labels`: what `bfs` (int32 depths) or `sssp` (float32 distances) delivered from `source`, a
    contiguous tensor of V on the context's device; the dtype selects grx_bfs_predecessors or
    grx_sssp_predecessors.  predecessors[v] is the smallest u with an entry (u, v, w) such that
    label[u] + 1 == label[v] (BFS) or label[u] + w == label[v] as one float32 add with label[u] <
    label[v] (SSSP); `source` for the source, -1 for an unreached vertex, -2 for an orphan (a reached
    vertex without such an entry: behind a zero or absorbed weight).  `violations` counts the entries
    with label[u] + w < label[v]: 0 exactly when the labels are a fixed point of relaxation, so the
    call doubles as a check of a result (include/essentials_amd.h has the definition).
    `predecessors`: int32 contiguous tensor of V on the context's device, allocated when None.
    `hops` (float32 labels only; True, or such an int32 tensor): the steps from each vertex to the
    source along the tree, -1 where the chain does not reach it; for int32 labels the depth is that
    number and hops=True raises ValueError.  The same call returns identical tensors.  Options read:
    collect_kernel_time.  Stats.pull_iterations is 1 when the pass walked in-rows and
    Stats.iterations the doubling rounds that `hops` took."""
    torch = _torch()
    device = torch.device(f"cuda:{ctx.device}")
    if not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.int32, torch.float32):
        raise TypeError("predecessors: labels must be an int32 or a float32 torch tensor")
    if labels.dim() != 1 or labels.numel() != g.n_rows or not labels.is_contiguous():
        raise ValueError(f"predecessors: labels must be a contiguous tensor of {g.n_rows} elements")
    if labels.device != device:
        raise ValueError(f"predecessors: labels must live on {device}")
    weighted = labels.dtype == torch.float32
    if hops is not None and hops is not False and not weighted:
        raise ValueError("predecessors: hops along a BFS tree are the depths; hops needs float32 labels")
    predecessors = _vertex_output(ctx, g, predecessors, "predecessors", "predecessors")
    if hops is None or hops is False:
        hops = None
    else:
        hops = _vertex_output(ctx, g, None if hops is True else hops, "predecessors", "hops")
    orphans, violations = C.c_int64(), C.c_int64()
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    lib = load_library()
    nonempty = g.n_rows > 0
    if weighted:
        _check(lib.grx_sssp_predecessors(ctx._h, g._h, source, _ptr(labels) if nonempty else None,
                                         _ptr(predecessors) if nonempty else None,
                                         _ptr(hops) if nonempty and hops is not None else None, C.byref(orphans),
                                         C.byref(violations), C.byref(o), C.byref(s)), "grx_sssp_predecessors")
    else:
        _check(lib.grx_bfs_predecessors(ctx._h, g._h, source, _ptr(labels) if nonempty else None,
                                        _ptr(predecessors) if nonempty else None, C.byref(orphans),
                                        C.byref(violations), C.byref(o), C.byref(s)), "grx_bfs_predecessors")
    return predecessors, hops, {"orphans": int(orphans.value), "violations": int(violations.value)}, Stats._from(s)


def path(predecessors, target: int) -> list:
    """The vertices from the source to `target`, both ends included, along `predecessors` (a torch
    tensor or a numpy array as `predecessors` returns it; copied to the host and walked there).  []
    when the chain from `target` does not end at a vertex that is its own predecessor: `target` is
    unreached, an orphan, behind one, or out of range.  At most V steps are made."""
    p = predecessors.detach().cpu().numpy() if hasattr(predecessors, "detach") else np.asarray(predecessors)
    n, v = len(p), int(target)
    if not 0 <= v < n:
        return []
    walked = [v]
    for _ in range(n):
        u = int(p[v])
        if u == v:
            return walked[::-1]
        if not 0 <= u < n:
            return []
        walked.append(u)
        v = u
    return []


def random_walk(ctx: Context, g: Graph, starts=None, length: int = 80, seed: int = 0, weighted: bool = False,
                p: float = 1.0, q: float = 1.0, walks_per_start: int = 1, walks=None,
                options: Optional[Options] = None):
    """Random walks, one lane per walk -> (int32 walks [count, length + 1] on the device, Stats).

    `starts`: None (every vertex), one vertex, or a sequence / numpy array of vertices, as `ppr` reads
    its seeds; a vertex named twice is two walks with different draws, and `walks_per_start` > 1
    repeats every start that many times, consecutively.  Row i is start_i, v_1, ..., v_length; a walk
    that meets a dead end (an empty row; when `weighted`, a row whose weights do not sum above 0)
    stops there and the rest of its row is -1.  `weighted`: entries are taken in proportion to their
    weights instead of uniformly.  `p`, `q` in [0.125, 8]: node2vec's return and in-out parameters, by
    rejection; with both 1 the walk is first-order.  Every draw is a function of (`seed`, i, step), so
    the same call returns the same tensor, and row i does not depend on what else is in the list
    (include/essentials_amd.h has the definition).  A directed graph is walked along its out-entries.
    `walks`: int32 contiguous tensor of count * (length + 1) elements on the context's device,
    allocated when None.  Options read: collect_kernel_time.  Stats.iterations is the longest walk's
    steps, Stats.vertices_reached the walks of full length, Stats.edges_traversed the steps taken,
    Stats.edges_expanded the candidates drawn and Stats.frontier_slots[t - 1] the walks that took
    step t."""
    torch = _torch()
    device = torch.device(f"cuda:{ctx.device}")
    if walks_per_start < 1:
        raise ValueError("random_walk: walks_per_start must be at least 1")
    if starts is None and walks_per_start == 1:
        h, n, count = None, 0, g.n_rows
    else:
        h = np.arange(g.n_rows) if starts is None else np.atleast_1d(np.asarray(starts))
        if h.ndim != 1:
            raise ValueError("random_walk: starts must be one vertex or a flat list of vertices")
        h = np.ascontiguousarray(np.repeat(h, walks_per_start), dtype=np.int32)
        n = count = int(h.size)
        if n == 0:  # an empty list is not "every vertex": hand the ABI a non-NULL pointer
            h = np.zeros(1, np.int32)
    width = int(length) + 1
    if walks is None:
        walks = torch.empty((count, max(width, 0)), dtype=torch.int32, device=device)
    else:
        if not isinstance(walks, torch.Tensor) or walks.dtype != torch.int32:
            raise TypeError("random_walk: walks must be an int32 torch tensor")
        if length < 0 or walks.numel() != count * width or not walks.is_contiguous():
            raise ValueError(f"random_walk: walks must be a contiguous tensor of {count} x {width} elements")
        if walks.device != device:
            raise ValueError(f"random_walk: walks must live on {device}")
        walks = walks.view(count, width)
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_random_walk(ctx._h, g._h, _ptr(h), n, length, seed, int(bool(weighted)), p, q,
                                          _ptr(walks) if walks.numel() else None, C.byref(o), C.byref(s)),
           "grx_random_walk")
    return walks, Stats._from(s)


@dataclass
class NeighborSample:
    """What `neighbor_sample` returns: int32 device tensors `nodes` (vertex ids in the graph's numbering,
    in local-id order), `src`, `dst` (local ids) and `entries` (positions in the column array), and the
    Python lists `node_offsets` (level L is nodes[node_offsets[L]:node_offsets[L + 1]]) and
    `edge_offsets` (hop h is [edge_offsets[h - 1], edge_offsets[h]))."""
    nodes: object
    src: object
    dst: object
    entries: object
    node_offsets: list
    edge_offsets: list


def neighbor_sample(ctx: Context, g: Graph, seeds=None, fanouts=(25, 10), seed: int = 0,
                    options: Optional[Options] = None):
    """Multi-hop fan-out neighbour sampling without replacement -> (NeighborSample, Stats).

    `seeds`: None (every vertex), one vertex, or a sequence / numpy array of vertices; repeats are
    dropped.  `fanouts`: per hop, at most that many entries of each expanded row (1..1024), or -1 for
    every entry.  Hop h expands the vertices first reached in hop h - 1; a vertex is expanded once.
    `nodes[src]`, `nodes[dst]` is the global edge list, and `torch.stack([dst, src])` is a PyG
    `edge_index` (messages flow from the sampled neighbour to the expanded vertex) into `x[nodes]`;
    `entries` indexes the graph's column and value arrays.  Every draw is a function of (`seed`, vertex,
    hop), so the same call returns the same tensors and a vertex's sample does not depend on the other
    seeds: vary `seed` per batch (include/essentials_amd.h has the definition).  A directed graph is
    sampled along its out-entries.  The tensors are allocated by the bounds that never fail and
    returned as slices of the true lengths.  Options read: collect_kernel_time.  Stats.iterations is
    the hops that expanded a vertex, Stats.vertices_reached the nodes, Stats.edges_traversed the sampled
    edges, Stats.edges_expanded the candidates drawn (a row taken whole counts its length) and
    Stats.frontier_slots[h - 1] the vertices expanded in hop h."""
    torch = _torch()
    device = torch.device(f"cuda:{ctx.device}")
    fan = np.ascontiguousarray(np.atleast_1d(np.asarray(fanouts)), dtype=np.int32)
    if fan.ndim != 1:
        raise ValueError("neighbor_sample: fanouts must be one fan-out or a flat list of them")
    hops = int(fan.size)
    if seeds is None:
        h, n, distinct = None, 0, g.n_rows
    else:
        h = np.atleast_1d(np.asarray(seeds))
        if h.ndim != 1:
            raise ValueError("neighbor_sample: seeds must be one vertex or a flat list of vertices")
        h = np.ascontiguousarray(h, dtype=np.int32)
        n, distinct = int(h.size), int(np.unique(h).size)
        if n == 0:  # an empty list is not "every vertex": hand the ABI a non-NULL pointer
            h = np.zeros(1, np.int32)
    # the bounds that never fail
    nnz, edge_cap, level = int(g.nnz), 0, distinct
    for k in fan.tolist():
        e = nnz if k < 1 else min(level * k, nnz)  # a bad fan-out is the ABI's to refuse
        edge_cap, level = edge_cap + e, min(e, g.n_rows)
    edge_cap = min(edge_cap, nnz)
    node_cap = min(distinct + edge_cap, g.n_rows)
    nodes = torch.empty(max(node_cap, 1), dtype=torch.int32, device=device)
    src, dst, entries = (torch.empty(max(edge_cap, 1), dtype=torch.int32, device=device) for _ in range(3))
    node_off = np.zeros(hops + 2, np.int64)
    edge_off = np.zeros(hops + 1, np.int64)
    o = (options or Options())._c()
    s = _Stats()
    ctx.after_torch()
    _check(load_library().grx_neighbor_sample(ctx._h, g._h, _ptr(h), n, _ptr(fan) if hops else None, hops, seed, _ptr(nodes), node_cap,
                                              _ptr(src), _ptr(dst), _ptr(entries), edge_cap, _ptr(node_off),
                                              _ptr(edge_off), C.byref(o), C.byref(s)), "grx_neighbor_sample")
    nn, ne = int(node_off[-1]), int(edge_off[-1])
    return NeighborSample(nodes[:nn], src[:ne], dst[:ne], entries[:ne], node_off.tolist(), edge_off.tolist()), \
        Stats._from(s)


def advance(ctx: Context, g: Graph, frontier, op: EdgeOp = EdgeOp.all, state=None, iparam: int = 0,
            options: Optional[Options] = None, want_output: bool = True,
            capacity: Optional[int] = None):
    """operators::advance::execute (frontier overload).  frontier=None -> whole graph.

    Returns the output frontier (int32 device tensor, order unspecified) or None.
    """
    torch = _torch()
    o = (options or Options())._c()
    n_in = 0 if frontier is None else frontier.numel()
    if frontier is not None and n_in == 0:
        # an EMPTY frontier is not "the whole graph": hand the ABI a non-NULL pointer
        frontier = torch.empty(1, dtype=torch.int32, device=f"cuda:{ctx.device}")
    out = None
    cap = 0
    if want_output:
        cap = capacity if capacity is not None else max(int(g.nnz) * 2 + 16, 16)
        out = torch.empty(cap, dtype=torch.int32, device=f"cuda:{ctx.device}")
    n_out = C.c_int64()
    ctx.after_torch()
    _check(load_library().grx_advance(ctx._h, g._h, C.byref(o), int(op), _ptr(state), iparam,
                                      _ptr(frontier), n_in, _ptr(out), cap, C.byref(n_out)),
           "grx_advance")
    return out[: n_out.value] if want_output else None


def filter(ctx: Context, g: Graph, frontier, algorithm: FilterAlgorithm,
           pred: VertexOp = VertexOp.all, state=None, iparam: int = 0):
    """operators::filter::execute (frontier overload) -> new frontier tensor."""
    torch = _torch()
    n_in = frontier.numel()
    out = torch.empty(max(n_in, 1), dtype=torch.int32, device=f"cuda:{ctx.device}")
    n_out = C.c_int64()
    ctx.after_torch()
    _check(load_library().grx_filter(ctx._h, g._h, int(algorithm), int(pred), _ptr(state), iparam,
                                     _ptr(frontier) if n_in else None, n_in, _ptr(out),
                                     out.numel(), C.byref(n_out)), "grx_filter")
    return out[: n_out.value]


def uniquify(ctx: Context, frontier, algorithm: UniquifyAlgorithm = UniquifyAlgorithm.unique,
             best_effort: bool = False):
    """operators::uniquify::execute (frontier overload) -> deduplicated frontier tensor."""
    torch = _torch()
    n_in = frontier.numel()
    work = frontier.clone()
    out = torch.empty(max(n_in, 1), dtype=torch.int32, device=f"cuda:{ctx.device}")
    n_out = C.c_int64()
    ctx.after_torch()
    _check(load_library().grx_uniquify(ctx._h, int(algorithm), int(best_effort),
                                       _ptr(work) if n_in else None, n_in, _ptr(out), out.numel(),
                                       C.byref(n_out)), "grx_uniquify")
    res = work if algorithm == UniquifyAlgorithm.unique else out
    return res[: n_out.value]

"""Python mirror of libbine's reduce-family operator interface on MI355X.

Every function named after a libbine entry point (reference include/libbine.h:
30-78) takes the same arguments in the same order --
``allreduce_bine_bdw_remap(sbuf, rbuf, count, dtype, op, comm)`` -- where the
buffers are device tensors (torch, ROCm) or raw device addresses, ``dtype`` is a
libbine element-type name ("float", "double", "int32", ...), one of the 16-bit
floating types "float16" | "bfloat16" (``EXT_DTYPES``: "sum" / "prod" / "max" /
"min" only, every pairwise reduction correctly rounded to the 16-bit format) or
a torch dtype (torch.float16 / torch.bfloat16 included),
``op`` is "sum" | "prod" | "max" | "min" | "land" | "lor" | "lxor" | "band" | "bor" | "bxor" |
"maxloc" | "minloc" (MPICH semantics; bitwise ops on integer types only, the loc ops on
the pair types "float_int" | "double_int" | "long_int" | "2int" | "short_int" only; the
complex types "c_float_complex" | "c_double_complex" under "sum" / "prod" only), and
``comm`` is a :class:`Comm`.
Errors raise :class:`BineError` carrying the status the reference would return
as an MPI error class.  The work runs in libbine_amd.so (HIP kernels + RCCL);
there is no fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

from . import _lib
from ._lib import ALGOS, DTYPES, EXT_DTYPES, OPS, BineError, check, lib

IN_PLACE = "IN_PLACE"   # libbine's MPI_IN_PLACE

_TORCH_DT = None


def _torch_dtypes():
    global _TORCH_DT
    if _TORCH_DT is None:
        import torch
        _TORCH_DT = {torch.float32: "float", torch.float64: "double", torch.int8: "int8",
                     torch.uint8: "uint8", torch.int16: "int16", torch.int32: "int32",
                     torch.int64: "int64", torch.float16: "float16", torch.bfloat16: "bfloat16"}
    return _TORCH_DT


def _dtype(dtype, *bufs) -> int:
    if dtype is None:
        for b in bufs:
            if hasattr(b, "dtype"):
                dtype = b.dtype
                break
    if not isinstance(dtype, str):
        dtype = _torch_dtypes()[dtype]
    return DTYPES[dtype] if dtype in DTYPES else EXT_DTYPES[dtype]


def _ptr(buf):
    if buf is None:
        return None
    if isinstance(buf, str) and buf == IN_PLACE:
        return _lib.IN_PLACE.value
    if hasattr(buf, "data_ptr"):
        return buf.data_ptr()
    return int(buf)


def _stream(stream, comm: Optional["Comm"]):
    if stream is not None:
        return stream if isinstance(stream, int) else getattr(stream, "cuda_stream", stream)
    try:
        import torch
        if torch.cuda.is_available():
            dev = comm.device if comm is not None else torch.cuda.current_device()
            return torch.cuda.current_stream(dev).cuda_stream
    except Exception:  # pragma: no cover
        pass
    return comm.stream if comm is not None else None


class Comm:
    """A bine communicator: one rank of an RCCL communicator (one process per
    GPU) or one virtual rank of an in-process loopback group."""

    def __init__(self, handle: int, kind: str):
        self.handle = ctypes.c_void_p(handle)
        self.kind = kind

    # -- construction --------------------------------------------------------
    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(_lib.UNIQUE_ID_BYTES)
        check(lib().bine_get_unique_id(buf), "bine_get_unique_id")
        return buf.raw

    @classmethod
    def rccl(cls, rank: int, size: int, unique_id: bytes, device: int = 0) -> "Comm":
        h = ctypes.c_void_p()
        idbuf = ctypes.create_string_buffer(unique_id, _lib.UNIQUE_ID_BYTES)
        check(lib().bine_comm_init_rccl(ctypes.byref(h), size, rank, idbuf, device), "bine_comm_init_rccl")
        return cls(h.value, "rccl")

    @classmethod
    def from_torch_distributed(cls, device: int, group=None) -> "Comm":
        """Bootstrap over an initialised torch.distributed group (any backend):
        rank 0 creates the RCCL unique id and broadcasts it."""
        import torch
        import torch.distributed as dist
        rank, size = dist.get_rank(group), dist.get_world_size(group)
        uid = cls.unique_id() if rank == 0 else bytes(_lib.UNIQUE_ID_BYTES)
        t = torch.tensor(list(uid), dtype=torch.uint8)
        if dist.get_backend(group) == "nccl":
            t = t.cuda(device)
        dist.broadcast(t, 0, group=group)
        return cls.rccl(rank, size, bytes(t.cpu().tolist()), device)

    @classmethod
    def loopback(cls, nranks: int, device: int = 0) -> list["Comm"]:
        arr = (ctypes.c_void_p * nranks)()
        check(lib().bine_comm_init_loopback(arr, nranks, device), "bine_comm_init_loopback")
        return [cls(arr[r], "loopback") for r in range(nranks)]

    # -- properties ----------------------------------------------------------
    @property
    def rank(self) -> int:
        return lib().bine_comm_rank(self.handle)

    @property
    def size(self) -> int:
        return lib().bine_comm_size(self.handle)

    @property
    def device(self) -> int:
        return lib().bine_comm_device(self.handle)

    @property
    def stream(self) -> int:
        return lib().bine_comm_stream(self.handle)

    def synchronize(self) -> None:
        check(lib().bine_comm_synchronize(self.handle), "bine_comm_synchronize")

    def set_trees(self, on: bool) -> None:
        """Multi-tree mode (allreduce, P = 4 / 8); collective."""
        check(lib().bine_comm_set_trees(self.handle, int(on)), "bine_comm_set_trees")

    def set_coll_a2a(self, on: bool) -> None:
        """RCCL communicators, relay / trees off: exchanges with one equal-sized
        message to and from every peer as one ncclAllToAllv; bit-identical."""
        check(lib().bine_comm_set_coll_a2a(self.handle, int(on)), "bine_comm_set_coll_a2a")

    def set_coll_ag(self, on: bool) -> None:
        """RCCL communicators: run one-buffer-to-all-peers exchanges (the flat
        allgather phase) as ncclAllGather + device copies; bit-identical."""
        check(lib().bine_comm_set_coll_ag(self.handle, int(on)), "bine_comm_set_coll_ag")

    def set_flat_ag(self, on) -> None:
        """Allreduce (remap / static, power-of-two P): one all-peers allgather
        exchange after the Bine reduce-scatter; bit-identical; collective.
        on = 2: with the flat reduce-scatter, the allgather is cut with its
        chunks (outputs complete chunk by chunk)."""
        check(lib().bine_comm_set_flat_ag(self.handle, int(on)), "bine_comm_set_flat_ag")

    def set_flat_rs(self, on: bool) -> None:
        """Flat reduce-scatter phase (one all-peers exchange + the reference's
        reduction tree in one kernel; bit-identical); collective."""
        check(lib().bine_comm_set_flat_rs(self.handle, int(on)), "bine_comm_set_flat_rs")

    def set_graphs(self, on: bool) -> None:
        """Graph mode (RCCL communicators): capture each (collective, buffers,
        stream) once into a HIP graph and replay it; bit-identical; the
        stream must not be the NULL stream."""
        check(lib().bine_comm_set_graphs(self.handle, int(on)), "bine_comm_set_graphs")

    def fused_calls(self) -> int:
        """large collectives issued as one k_dm_fused launch (bine_comm_fused_calls)"""
        n = lib().bine_comm_fused_calls(self.handle)
        if n < 0:
            check(int(-n), "bine_comm_fused_calls")
        return int(n)

    def graphs_cached(self) -> int:
        """graphs graph mode holds (0: every call so far ran eagerly)"""
        n = lib().bine_comm_graphs_cached(self.handle)
        if n < 0:
            check(int(-n), "bine_comm_graphs_cached")
        return int(n)

    def set_direct(self, on: bool) -> None:
        """RCCL communicators on one node: exchanges through mapped peer memory
        (bine_comm_set_direct); bit-identical.  EVERY call with on=True is
        collective (all ranks, same point: set-up, or the rebuild of a
        transport a timeout disabled on any rank); on=False is local."""
        check(lib().bine_comm_set_direct(self.handle, int(on)), "bine_comm_set_direct")

    def set_direct_wgs(self, wgs: int) -> None:
        """workgroups per message of the direct transport (0 = default;
        bine_comm_set_direct_wgs); local, drops cached graphs"""
        check(lib().bine_comm_set_direct_wgs(self.handle, int(wgs)), "bine_comm_set_direct_wgs")

    def set_direct_tree(self, on) -> None:
        """direct transport: the flat reduce-scatter's trees inside the exchange
        launches (bine_comm_set_direct_tree; -1 = BINE_DIRECT_TREE); every rank
        alike; bit-identical"""
        check(lib().bine_comm_set_direct_tree(self.handle, int(on)), "bine_comm_set_direct_tree")

    def direct_timed_out(self) -> bool:
        """a wait of this rank's direct transport timed out (bine_comm_direct_timed_out)"""
        n = lib().bine_comm_direct_timed_out(self.handle)
        if n < 0:
            check(int(-n), "bine_comm_direct_timed_out")
        return bool(n)

    def direct_ping(self, peer: int, iters: int = 1000) -> float:
        """microseconds per cross-GPU flag round trip with `peer` over the
        direct transport (bine_comm_direct_ping; both ranks call it together)"""
        us = ctypes.c_double(0.0)
        check(lib().bine_comm_direct_ping(self.handle, peer, iters, ctypes.byref(us)), "bine_comm_direct_ping")
        return us.value

    def direct_stamps(self, reset: bool = True):
        """Direct-transport diagnostics (BINE_DIRECT_STAMPS=<records> at setup;
        bine_comm_direct_stamps): numpy uint64 array (n, 4) of per-workgroup
        records -- tag (serial << 32 | kind << 24 | msg << 16 | wg; kind 0 push,
        1 pull, 2 tree), wall_clock64 at entry, wait done, copy done."""
        import numpy as np
        n = ctypes.c_size_t(0)
        check(lib().bine_comm_direct_stamps(self.handle, None, 0, ctypes.byref(n), 0), "bine_comm_direct_stamps")
        out = np.zeros((max(int(n.value), 1), 4), dtype=np.uint64)
        check(lib().bine_comm_direct_stamps(self.handle, out.ctypes.data, int(n.value), ctypes.byref(n),
                                            int(reset)), "bine_comm_direct_stamps")
        return out[:min(int(n.value), out.shape[0])] if n.value else out[:0]

    def set_profile(self, on: bool) -> None:
        """Per-op device timing of the following collectives (bine_comm_set_profile)."""
        check(lib().bine_comm_set_profile(self.handle, int(on)), "bine_comm_set_profile")

    def profile(self):
        """Per-op timing of the latest profiled collective: list of
        {"xchg", "nprims", "bytes", "start_ms", "ms"} in issue order."""
        n = lib().bine_comm_profile(self.handle, None, 0)
        if n < 0:
            raise BineError(int(-n), "bine_comm_profile")
        arr = (_lib.OpTime * max(int(n), 1))()
        n = lib().bine_comm_profile(self.handle, arr, n)
        if n < 0:
            raise BineError(int(-n), "bine_comm_profile")
        return [{f: getattr(arr[k], f) for f, _ in _lib.OpTime._fields_} for k in range(int(n))]

    def set_chunk(self, nbytes: int) -> None:
        """Pipelining chunk in bytes (0 = default 16 MiB); never changes a bit; collective."""
        check(lib().bine_comm_set_chunk(self.handle, nbytes), "bine_comm_set_chunk")

    def set_relay(self, min_part_bytes: int) -> None:
        """Multi-link relay for permutation steps (0 = off); collective."""
        check(lib().bine_comm_set_relay(self.handle, min_part_bytes), "bine_comm_set_relay")

    def destroy(self) -> None:
        if self.handle:
            lib().bine_comm_destroy(self.handle)
            self.handle = ctypes.c_void_p()


# ---- arithmetic boundary ------------------------------------------------------

def reduce_local(inbuf, inoutbuf, count: int, dtype=None, op: str = "sum", stream=None) -> None:
    """MPI_Reduce_local on the GPU: inout = inout (op) in."""
    check(lib().bine_reduce_local(_ptr(inbuf), _ptr(inoutbuf), count, _dtype(dtype, inbuf), OPS[op],
                                  _stream(stream, None)), "bine_reduce_local")


def reduce3(a, b, out, count: int, dtype=None, op: str = "sum", stream=None) -> None:
    """out = b (op) a (out may alias b)."""
    check(lib().bine_reduce3(_ptr(a), _ptr(b), _ptr(out), count, _dtype(dtype, a), OPS[op],
                             _stream(stream, None)), "bine_reduce3")


def fill_pico(buf, count: int, dtype=None, seed: int = 1234, stream=None) -> None:
    """pico_core's rand_r() input distribution, generated on the device."""
    check(lib().bine_fill_pico(_ptr(buf), count, _dtype(dtype, buf), seed, _stream(stream, None)),
          "bine_fill_pico")


def copy(dst, src, nbytes: int, stream=None) -> None:
    """copy_buffer on the device (bine_copy: the k_copy kernel every COPY
    primitive runs)."""
    check(lib().bine_copy(_ptr(dst), _ptr(src), nbytes, _stream(stream, None)), "bine_copy")


def rccl_version() -> dict:
    """{"runtime": code, "compiled": code, ..., "abi_ok"}: the RCCL this process
    maps vs the headers libbine_amd.so was compiled against (NCCL_VERSION
    codes), and whether the pair lies in the checked ABI window -- reported
    also when it does not (communicator creation refuses such a pair)."""
    rt, ct = ctypes.c_int(), ctypes.c_int()
    check(lib().bine_rccl_version(ctypes.byref(rt), ctypes.byref(ct)), "bine_rccl_version")

    def fmt(v):
        return f"{v // 10000}.{v // 100 % 100}.{v % 100}"
    return {"runtime": fmt(rt.value), "compiled": fmt(ct.value), "runtime_code": rt.value,
            "compiled_code": ct.value, "abi_ok": lib().bine_rccl_abi_check(rt.value, ct.value) == 0}


def checksum(buf, count: int, dtype=None, stream=None) -> int:
    out = ctypes.c_uint64()
    check(lib().bine_checksum(_ptr(buf), count, _dtype(dtype, buf), ctypes.byref(out), _stream(stream, None)),
          "bine_checksum")
    return out.value


def set_reduce_tuning(unroll: int = 4, maxblocks: int = 0, nontemporal: int = 1) -> None:
    """bine_set_reduce_tuning; with no argument, the library's defaults."""
    lib().bine_set_reduce_tuning(unroll, maxblocks, nontemporal)


# ---- generic collectives -------------------------------------------------------

def _algo(coll: str, algo) -> int:
    return algo if isinstance(algo, int) else ALGOS[coll][algo]


def _scaled(op: str, scale, comm: Comm):
    """(op, scale) of a call: op="avg" is op="sum" with scale = 1 / comm.size
    (resolved here; the C op table has no such op)."""
    if op == "avg":
        if scale is not None:
            raise ValueError('op="avg" is op="sum", scale=1/comm.size: pass no scale of your own')
        return "sum", 1.0 / comm.size
    return op, scale


def scale(inbuf, outbuf, count: int, dtype=None, scale: float = 1.0, stream=None) -> None:
    """out[i] = S(in[i]) (bine_scale): one multiplication by `scale` as the
    scaled collectives define it -- float / double in their own format; float16
    / bfloat16 widened to binary32, multiplied by float32(scale), rounded to
    nearest even.  outbuf may be inbuf."""
    check(lib().bine_scale(_ptr(inbuf), _ptr(outbuf), count, _dtype(dtype, outbuf), float(scale),
                           _stream(stream, None)), "bine_scale")


def scale_valid(dtype, op: str) -> bool:
    """whether the scaled calls accept (dtype, op): the four floating types
    with sum / prod / max / min (bine_scale_valid)"""
    return bool(lib().bine_scale_valid(_dtype(dtype), OPS[op]))


def allreduce(algo, sbuf, rbuf, count: int, dtype, op: str, comm: Comm, segsize: int = 0, stream=None,
              scale=None) -> None:
    """scale: the result times `scale` (bine_allreduce_scaled; op="avg": the
    mean, sum times 1 / comm.size), fused into the flat forms' tree kernels"""
    op, scale = _scaled(op, scale, comm)
    if scale is not None:
        check(lib().bine_allreduce_scaled(comm.handle, _algo("allreduce", algo), _ptr(sbuf), _ptr(rbuf), count,
                                          _dtype(dtype, rbuf), OPS[op], float(scale), segsize,
                                          _stream(stream, comm)), f"allreduce_{algo} (scaled)")
        return
    check(lib().bine_allreduce(comm.handle, _algo("allreduce", algo), _ptr(sbuf), _ptr(rbuf), count,
                               _dtype(dtype, rbuf), OPS[op], segsize, _stream(stream, comm)), f"allreduce_{algo}")


def reduce_scatter(algo, sbuf, rbuf, rcounts: Sequence[int], dtype, op: str, comm: Comm, stream=None,
                   scale=None) -> None:
    """scale: as allreduce's (bine_reduce_scatter_scaled)"""
    rc = (ctypes.c_int * len(rcounts))(*rcounts)
    op, scale = _scaled(op, scale, comm)
    if scale is not None:
        check(lib().bine_reduce_scatter_scaled(comm.handle, _algo("reduce_scatter", algo), _ptr(sbuf), _ptr(rbuf),
                                               rc, _dtype(dtype, rbuf), OPS[op], float(scale),
                                               _stream(stream, comm)), f"reduce_scatter_{algo} (scaled)")
        return
    check(lib().bine_reduce_scatter(comm.handle, _algo("reduce_scatter", algo), _ptr(sbuf), _ptr(rbuf), rc,
                                    _dtype(dtype, rbuf), OPS[op], _stream(stream, comm)), f"reduce_scatter_{algo}")


# ---- wide (binary32-accumulating) forms of the 16-bit types ---------------------

def wide_valid(dtype, op: str) -> bool:
    """whether the wide calls accept (dtype, op): float16 / bfloat16 with sum /
    prod / max / min (bine_wide_valid)"""
    return bool(lib().bine_wide_valid(_dtype(dtype), OPS[op]))


def widen(inbuf, outbuf, count: int, dtype=None, stream=None) -> None:
    """outbuf (float32)[i] = inbuf (float16 / bfloat16)[i], exactly (bine_widen)"""
    check(lib().bine_widen(_ptr(inbuf), _ptr(outbuf), count, _dtype(dtype, inbuf), _stream(stream, None)),
          "bine_widen")


def narrow(inbuf, outbuf, count: int, dtype=None, stream=None) -> None:
    """outbuf (float16 / bfloat16)[i] = inbuf (float32)[i] rounded to nearest even
    (bine_narrow)"""
    check(lib().bine_narrow(_ptr(inbuf), _ptr(outbuf), count, _dtype(dtype, outbuf), _stream(stream, None)),
          "bine_narrow")


def reduce_tree_wide(leaves, out, count: int, dtype, op: str = "sum", stream=None, swap: int = 0,
                     scale: float = 1.0) -> int:
    """bine_reduce_tree_wide: the tree over the 16-bit leaves evaluated in
    binary32, times float32(scale), narrowed once.  Returns the status."""
    return lib().bine_reduce_tree_wide(len(leaves), _ptrs(leaves), _ptr(out), count, _dtype(dtype, out), OPS[op],
                                       swap, float(scale), _stream(stream, None))


def _wide_scale(op: str, scale, comm: Comm):
    op, scale = _scaled(op, scale, comm)
    return op, 1.0 if scale is None else float(scale)


def allreduce_wide(algo, sbuf, rbuf, count: int, dtype, op: str, comm: Comm, segsize: int = 0, stream=None,
                   scale=None) -> None:
    """bine_allreduce_wide: float16 / bfloat16 buffers, every pairwise reduction
    in binary32, one rounding to 16 bits per output element; scale / op="avg"
    as allreduce's"""
    op, scale = _wide_scale(op, scale, comm)
    check(lib().bine_allreduce_wide(comm.handle, _algo("allreduce", algo), _ptr(sbuf), _ptr(rbuf), count,
                                    _dtype(dtype, rbuf), OPS[op], scale, segsize, _stream(stream, comm)),
          f"allreduce_{algo} (wide)")


def reduce_scatter_wide(algo, sbuf, rbuf, rcounts: Sequence[int], dtype, op: str, comm: Comm, stream=None,
                        scale=None) -> None:
    """bine_reduce_scatter_wide (see allreduce_wide)"""
    rc = (ctypes.c_int * len(rcounts))(*rcounts)
    op, scale = _wide_scale(op, scale, comm)
    check(lib().bine_reduce_scatter_wide(comm.handle, _algo("reduce_scatter", algo), _ptr(sbuf), _ptr(rbuf), rc,
                                         _dtype(dtype, rbuf), OPS[op], scale, _stream(stream, comm)),
          f"reduce_scatter_{algo} (wide)")


def loopback_allreduce_wide(comms, algo, sbufs, rbufs, count, dtype, op="sum", segsize=0, scale=None):
    st = (ctypes.c_int * len(comms))()
    hs = (ctypes.c_void_p * len(comms))(*[c.handle.value for c in comms])
    op, scale = _wide_scale(op, scale, comms[0])
    rc = lib().bine_loopback_run_allreduce_wide(hs, len(comms), _algo("allreduce", algo), _ptrs(sbufs), _ptrs(rbufs),
                                                count, _dtype(dtype, rbufs[0]), OPS[op], scale, segsize, st)
    return rc, list(st)


def loopback_reduce_scatter_wide(comms, algo, sbufs, rbufs, rcounts, dtype, op="sum", scale=None):
    st = (ctypes.c_int * len(comms))()
    hs = (ctypes.c_void_p * len(comms))(*[c.handle.value for c in comms])
    rcs = (ctypes.c_int * len(rcounts))(*rcounts)
    op, scale = _wide_scale(op, scale, comms[0])
    rc = lib().bine_loopback_run_reduce_scatter_wide(hs, len(comms), _algo("reduce_scatter", algo), _ptrs(sbufs),
                                                     _ptrs(rbufs), rcs, _dtype(dtype, rbufs[0]), OPS[op], scale, st)
    return rc, list(st)


def wide_plan(coll: str, algo, nranks: int, count: int = 0, rcounts=None, trees: bool = False,
              flat_ag=False, flat_rs: bool = False) -> bool:
    """Which path a wide call takes (bine_plan_wide, host only): True = path B
    (the 16-bit plan with BINE_PRIM_WIDE trees), False = path A (through
    binary32).  Raises BineError where the call's plan fails."""
    rc = (ctypes.c_int * nranks)(*rcounts) if rcounts is not None else None
    mode = int(trees) | (2 if flat_ag else 0) | (4 if flat_rs else 0) | (8 if flat_ag == 2 else 0)
    r = lib().bine_plan_wide(_algo(coll, algo), nranks, count, rc, mode)
    if r < 0:
        raise BineError(-r, f"wide_plan {coll}_{algo}")
    return bool(r)


# ---- multi-buffer forms: many tensors, one call ------------------------------------

def copy_segments(dsts, srcs, nbytes: Sequence[int], stream=None) -> None:
    """dsts[k][:nbytes[k]] = srcs[k][:nbytes[k]] for every k (bytes), all in
    ceil(non-empty / COPY_SEGS_PER_LAUNCH) launches of k_copy_segs
    (bine_copy_segments).  Any alignment; empty segments may be None; the
    destination ranges must not overlap each other or any source range."""
    n = len(nbytes)
    if len(dsts) != n or len(srcs) != n:
        raise ValueError("copy_segments: dsts, srcs and nbytes differ in length")
    check(lib().bine_copy_segments(n, _ptrs(dsts), _ptrs(srcs), (ctypes.c_size_t * max(n, 1))(*nbytes),
                                   _stream(stream, None)), "bine_copy_segments")


def plan_segments(dst_addrs: Sequence[int], src_addrs: Sequence[int], nbytes: Sequence[int]):
    """The tile table of that call (bine_plan_segments, host only): a list of
    (launch, segment, byte offset in the segment, bytes, kind), kind 0 = a
    vector tile, 1 = head / tail bytes."""
    n = len(nbytes)
    d = (ctypes.c_uint64 * max(n, 1))(*dst_addrs)
    s = (ctypes.c_uint64 * max(n, 1))(*src_addrs)
    b = (ctypes.c_size_t * max(n, 1))(*nbytes)
    nt = lib().bine_plan_segments(n, d, s, b, None, 0)
    if nt < 0:
        raise BineError(int(-nt), "bine_plan_segments")
    out = (ctypes.c_uint64 * max(5 * int(nt), 1))()
    lib().bine_plan_segments(n, d, s, b, out, nt)
    return [tuple(int(x) for x in out[5 * k:5 * k + 5]) for k in range(int(nt))]


def _multi_counts(rbufs, counts):
    if counts is None:
        counts = [b.numel() for b in rbufs]
    if len(counts) != len(rbufs):
        raise ValueError("allreduce_multi: counts and rbufs differ in length")
    return (ctypes.c_size_t * max(len(counts), 1))(*counts)


def _multi_family(op: str, scale, wide: bool, comm: Comm):
    """(op, the C call's scale): op="avg" through _scaled; no scale = 1.0, the
    unscaled call (wide=False) or the wide call times one"""
    op, scale = _scaled(op, scale, comm)
    return op, 1.0 if scale is None else float(scale)


def allreduce_multi(algo, sbufs, rbufs, dtype, op: str, comm: Comm, counts=None, segsize: int = 0, stream=None,
                    scale=None, wide: bool = False) -> None:
    """bine_allreduce_multi: the tensors of `rbufs` receive the slices of ONE
    allreduce over the concatenation of `sbufs`, bit for bit what allreduce /
    allreduce (scale=) / allreduce_wide (wide=True) gives in place on
    torch.cat(sbufs).  sbufs=None: every tensor in place; sbufs[k] is
    rbufs[k] or IN_PLACE: tensor k in place.  counts (elements, the same on
    every rank) defaults to each rbuf's numel()."""
    if sbufs is not None and len(sbufs) != len(rbufs):
        raise ValueError("allreduce_multi: sbufs and rbufs differ in length")
    op, scale = _multi_family(op, scale, wide, comm)
    c = _multi_counts(rbufs, counts)
    check(lib().bine_allreduce_multi(comm.handle, _algo("allreduce", algo), len(rbufs),
                                     None if sbufs is None else _ptrs(sbufs), _ptrs(rbufs), c,
                                     _dtype(dtype, *rbufs), OPS[op], scale, int(bool(wide)), segsize,
                                     _stream(stream, comm)), f"allreduce_{algo} (multi)")


def loopback_allreduce_multi(comms, algo, sbufs, rbufs, dtype, op="sum", counts=None, segsize=0, scale=None,
                             wide=False):
    """sbufs (None: in place) / rbufs: one list of tensors per virtual rank.
    Returns (status, per-rank statuses)."""
    st = (ctypes.c_int * len(comms))()
    hs = (ctypes.c_void_p * len(comms))(*[c.handle.value for c in comms])
    op, scale = _multi_family(op, scale, wide, comms[0])
    n = len(rbufs[0])
    if any(len(r) != n for r in rbufs) or (sbufs is not None and any(len(s) != n for s in sbufs)):
        raise ValueError("loopback_allreduce_multi: the ranks' lists differ in length")
    c = _multi_counts(rbufs[0], counts)
    flat_r = [b for r in rbufs for b in r]
    flat_s = None if sbufs is None else _ptrs([b for s in sbufs for b in s])
    rc = lib().bine_loopback_run_allreduce_multi(hs, len(comms), _algo("allreduce", algo), n, flat_s,
                                                 _ptrs(flat_r), c, _dtype(dtype, *flat_r), OPS[op], scale,
                                                 int(bool(wide)), segsize, st)
    return rc, list(st)


# ---- sharded multi-buffer forms: reduce-scatter / allgather of a bucket ----------------

def copy_shards(packed, flat, shard_bytes: Sequence[int], nranks: int, dir: int, stream=None) -> None:
    """All `nranks` shards of every tensor copied between the flat layout (shard
    j of tensor k at flat[k] + j * shard_bytes[k]) and the packed one (at packed
    + j * sum(shard_bytes) + the prefix sum of shard_bytes before k), in
    ceil(non-empty / COPY_SEGS_PER_LAUNCH) launches of k_copy_shards
    (bine_copy_shards).  dir 0: flat -> packed, dir 1: packed -> flat.  Any
    alignment; empty tensors may be None."""
    n = len(shard_bytes)
    if len(flat) != n:
        raise ValueError("copy_shards: flat and shard_bytes differ in length")
    check(lib().bine_copy_shards(n, nranks, dir, _ptr(packed), _ptrs(flat),
                                 (ctypes.c_size_t * max(n, 1))(*shard_bytes), _stream(stream, None)),
          "bine_copy_shards")


def plan_shards(packed_addr: int, flat_addrs: Sequence[int], shard_bytes: Sequence[int], nranks: int, dir: int):
    """The tile table of that call (bine_plan_shards, host only): a list of
    (launch, tensor, shard, byte offset in the shard, bytes, kind), kind 0 = a
    vector tile, 1 = head / tail bytes; only tiles that copy bytes."""
    n = len(shard_bytes)
    if len(flat_addrs) != n:
        raise ValueError("plan_shards: flat_addrs and shard_bytes differ in length")
    f = (ctypes.c_uint64 * max(n, 1))(*flat_addrs)
    b = (ctypes.c_size_t * max(n, 1))(*shard_bytes)
    nt = lib().bine_plan_shards(n, nranks, dir, packed_addr, f, b, None, 0)
    if nt < 0:
        raise BineError(int(-nt), "bine_plan_shards")
    out = (ctypes.c_uint64 * max(6 * int(nt), 1))()
    lib().bine_plan_shards(n, nranks, dir, packed_addr, f, b, out, nt)
    return [tuple(int(x) for x in out[6 * k:6 * k + 6]) for k in range(int(nt))]


def _shard_counts(name: str, rbufs, shard_counts, per: int):
    """shard_counts=None: each rbuf's numel() // per (reduce-scatter: per = 1,
    rbufs[k] IS a shard; allgather: per = comm.size, rbufs[k] holds them all)"""
    if shard_counts is None:
        shard_counts = []
        for b in rbufs:
            if b.numel() % per:
                raise ValueError(f"{name}: a tensor of {b.numel()} elements does not split into {per} equal shards")
            shard_counts.append(b.numel() // per)
    if len(shard_counts) != len(rbufs):
        raise ValueError(f"{name}: shard_counts and rbufs differ in length")
    return (ctypes.c_size_t * max(len(shard_counts), 1))(*shard_counts)


def reduce_scatter_multi(algo, sbufs, rbufs, dtype, op: str, comm: Comm, shard_counts=None, stream=None,
                         scale=None, wide: bool = False) -> None:
    """bine_reduce_scatter_multi: sbufs[k] holds comm.size shards of
    shard_counts[k] elements, rbufs[k] receives this rank's reduced shard --
    the slices of ONE reduce_scatter (scale= / op="avg": the scaled call,
    wide=True: reduce_scatter_wide) on the rank-major packing of the shards,
    bit for bit.  rbufs[k] may overlap sbufs[k].  shard_counts (the same on
    every rank) defaults to each rbuf's numel()."""
    if sbufs is None or len(sbufs) != len(rbufs):
        raise ValueError("reduce_scatter_multi: sbufs and rbufs differ in length")
    op, scale = _multi_family(op, scale, wide, comm)
    c = _shard_counts("reduce_scatter_multi", rbufs, shard_counts, 1)
    check(lib().bine_reduce_scatter_multi(comm.handle, _algo("reduce_scatter", algo), len(rbufs), _ptrs(sbufs),
                                          _ptrs(rbufs), c, _dtype(dtype, *rbufs), OPS[op], scale, int(bool(wide)),
                                          _stream(stream, comm)), f"reduce_scatter_{algo} (multi)")


def allgather_multi(algo, sbufs, rbufs, dtype, comm: Comm, shard_counts=None, stream=None) -> None:
    """bine_allgather_multi: rbufs[k][j * c : (j + 1) * c] = rank j's sbufs[k]
    (c = shard_counts[k] elements) for every tensor, as ONE allgather.
    sbufs=None, or sbufs[k] IN_PLACE: tensor k's input is its own shard's place
    in rbufs[k]; sbufs[k] may be any view into rbufs[k].  shard_counts (the
    same on every rank) defaults to each rbuf's numel() // comm.size."""
    if sbufs is not None and len(sbufs) != len(rbufs):
        raise ValueError("allgather_multi: sbufs and rbufs differ in length")
    c = _shard_counts("allgather_multi", rbufs, shard_counts, 1 if shard_counts is not None else comm.size)
    check(lib().bine_allgather_multi(comm.handle, _algo("allgather", algo), len(rbufs),
                                     None if sbufs is None else _ptrs(sbufs), _ptrs(rbufs), c,
                                     _dtype(dtype, *rbufs), _stream(stream, comm)), f"allgather_{algo} (multi)")


def _rank_lists(name: str, sbufs, rbufs):
    n = len(rbufs[0])
    if any(len(r) != n for r in rbufs) or (sbufs is not None and any(len(s) != n for s in sbufs)):
        raise ValueError(f"{name}: the ranks' lists differ in length")
    flat_r = [b for r in rbufs for b in r]
    return n, flat_r, None if sbufs is None else _ptrs([b for s in sbufs for b in s])


def loopback_reduce_scatter_multi(comms, algo, sbufs, rbufs, dtype, op="sum", shard_counts=None, scale=None,
                                  wide=False):
    """sbufs / rbufs: one list of tensors per virtual rank.  Returns (status,
    per-rank statuses)."""
    st = (ctypes.c_int * len(comms))()
    hs = (ctypes.c_void_p * len(comms))(*[c.handle.value for c in comms])
    op, scale = _multi_family(op, scale, wide, comms[0])
    n, flat_r, flat_s = _rank_lists("loopback_reduce_scatter_multi", sbufs, rbufs)
    c = _shard_counts("loopback_reduce_scatter_multi", rbufs[0], shard_counts, 1)
    rc = lib().bine_loopback_run_reduce_scatter_multi(hs, len(comms), _algo("reduce_scatter", algo), n, flat_s,
                                                      _ptrs(flat_r), c, _dtype(dtype, *flat_r), OPS[op], scale,
                                                      int(bool(wide)), st)
    return rc, list(st)


def loopback_allgather_multi(comms, algo, sbufs, rbufs, dtype, shard_counts=None):
    """sbufs (None: in place) / rbufs: one list of tensors per virtual rank.
    Returns (status, per-rank statuses)."""
    st = (ctypes.c_int * len(comms))()
    hs = (ctypes.c_void_p * len(comms))(*[c.handle.value for c in comms])
    n, flat_r, flat_s = _rank_lists("loopback_allgather_multi", sbufs, rbufs)
    c = _shard_counts("loopback_allgather_multi", rbufs[0], shard_counts,
                      1 if shard_counts is not None else len(comms))
    rc = lib().bine_loopback_run_allgather_multi(hs, len(comms), _algo("allgather", algo), n, flat_s, _ptrs(flat_r),
                                                 c, _dtype(dtype, *flat_r), st)
    return rc, list(st)


# ---- global norm and clipping of a bucket --------------------------------------------------

def _norm_counts(name: str, bufs, counts):
    """counts=None: each tensor's numel()"""
    if counts is None:
        counts = [b.numel() for b in bufs]
    if len(counts) != len(bufs):
        raise ValueError(f"{name}: counts and bufs differ in length")
    return (ctypes.c_size_t * max(len(counts), 1))(*counts)


def _norm_dtype(dtype, bufs) -> int:
    return dtype if isinstance(dtype, int) else _dtype(dtype, *bufs)


def plan_sumsq(addrs: Sequence[int], counts: Sequence[int], dtype) -> int:
    """The doubles of scratch sumsq_segments needs for these device addresses,
    element counts and dtype (bine_plan_sumsq, host only): one per workgroup,
    a workgroup per 32 KiB tile of 16-B aligned vectors and at least one per
    non-empty tensor."""
    n = len(counts)
    if len(addrs) != n:
        raise ValueError("plan_sumsq: addrs and counts differ in length")
    r = lib().bine_plan_sumsq(n, (ctypes.c_uint64 * max(n, 1))(*addrs), (ctypes.c_size_t * max(n, 1))(*counts),
                              _norm_dtype(dtype, ()))
    if r < 0:
        raise BineError(int(-r), "bine_plan_sumsq")
    return int(r)


def sumsq_segments(bufs, dtype=None, counts=None, out=None, scratch=None, scratch_doubles=None, stream=None):
    """out[k] = the sum of tensor k's squares in binary64, out[n] = out[0] + ... +
    out[n - 1] (bine_sumsq_segments): deterministic bits, relative error at most
    counts[k] * 2^-52.  float / double / float16 / bfloat16; empty tensors may be
    None.  `out` (n + 1 float64) and `scratch` (plan_sumsq(...) float64; a raw
    address needs scratch_doubles) are allocated with torch when not given.
    Returns out."""
    n = len(bufs)
    c = _norm_counts("sumsq_segments", bufs, counts)
    dt = _norm_dtype(dtype, bufs)
    if out is None or scratch is None:
        import torch
        dev = next((b.device for b in bufs if hasattr(b, "device")), "cuda")
        if out is None:
            out = torch.empty(n + 1, dtype=torch.float64, device=dev)
        if scratch is None:
            need = plan_sumsq([_ptr(b) or 0 for b in bufs], list(c)[:n], dt)
            scratch = torch.empty(max(need, 1), dtype=torch.float64, device=dev)
    if scratch_doubles is None:
        scratch_doubles = scratch.numel() if hasattr(scratch, "numel") else 0
    check(lib().bine_sumsq_segments(n, _ptrs(bufs), c, dt, _ptr(out), _ptr(scratch), scratch_doubles,
                                    _stream(stream, None)), "bine_sumsq_segments")
    return out


def clip_segments(bufs, norm2, max_norm: float, eps: float = 0.0, dtype=None, counts=None, coef_out=None,
                  stream=None) -> None:
    """Every tensor scaled in place by c = min(1, max_norm / (sqrt(norm2[0]) +
    eps)), computed on the device in binary64 from the device double `norm2`
    (bine_clip_segments); coef_out (a device double, optional) receives c.
    The multiplication is scale()'s, per element type; c == 1 changes nothing."""
    c = _norm_counts("clip_segments", bufs, counts)
    check(lib().bine_clip_segments(len(bufs), _ptrs(bufs), c, _norm_dtype(dtype, bufs), _ptr(norm2), float(max_norm),
                                   float(eps), _ptr(coef_out), _stream(stream, None)), "bine_clip_segments")


def _stats(bufs, stats, extra: int):
    if stats is None:
        import torch
        dev = next((b.device for b in bufs if hasattr(b, "device")), "cuda")
        stats = torch.empty(len(bufs) + extra, dtype=torch.float64, device=dev)
    return stats


def norm_multi(algo, bufs, dtype, comm: Comm, counts=None, stats=None, stream=None):
    """bine_norm_multi: stats[k] = tensor k's sum of squares over all ranks,
    stats[n] = the bucket's -- bit for bit ONE in-place allreduce (double, sum)
    of the ranks' sumsq_segments vectors.  Every rank passes the same number of
    tensors; counts may differ per rank.  A latency algorithm ("bine_lat",
    "recursivedoubling") is the intended choice.  stats: n + 1 float64 on the
    device (allocated when None).  Returns stats."""
    stats = _stats(bufs, stats, 1)
    c = _norm_counts("norm_multi", bufs, counts)
    check(lib().bine_norm_multi(comm.handle, _algo("allreduce", algo), len(bufs), _ptrs(bufs), c,
                                _norm_dtype(dtype, bufs), _ptr(stats), _stream(stream, comm)),
          f"norm_multi ({algo})")
    return stats


def _coef_only_args(name: str, max_norm, eps) -> None:
    """scale=False has no C call of its own to refuse these before the exchange"""
    if not float(max_norm) >= 0.0 or not float(eps) >= 0.0:
        raise BineError(1, f"{name}: max_norm or eps negative or NaN")


def clip_multi(algo, bufs, dtype, comm: Comm, max_norm: float, eps: float = 0.0, counts=None, stats=None,
               stream=None, scale: bool = True):
    """bine_clip_multi: norm_multi into stats[0..n], then every tensor scaled in
    place by c = min(1, max_norm / (sqrt(stats[n]) + eps)) (clip_segments);
    stats[n + 1] = c, the same bits on every rank.  stats: n + 2 float64.
    scale=False: the same statistics and coefficient, no tensor touched --
    norm_multi, then clip_segments on an empty list with norm2 = &stats[n],
    coef_out = &stats[n + 1].  That is the form to put in front of adamw_multi
    (gcoef=stats[n + 1:]), which applies the coefficient itself: after
    scale=True the gradient is clipped already and gcoef must stay None, or the
    coefficient is applied twice.  (max_norm and eps are refused first then.)
    Returns stats."""
    stats = _stats(bufs, stats, 2)
    if not scale:
        _coef_only_args("clip_multi", max_norm, eps)
        norm_multi(algo, bufs, dtype, comm, counts=counts, stats=stats, stream=stream)
        a = _ptr(stats)
        clip_segments([], a + 8 * len(bufs), max_norm, eps, dtype=_norm_dtype(dtype, bufs), counts=[],
                      coef_out=a + 8 * (len(bufs) + 1), stream=_stream(stream, comm))
        return stats
    c = _norm_counts("clip_multi", bufs, counts)
    check(lib().bine_clip_multi(comm.handle, _algo("allreduce", algo), len(bufs), _ptrs(bufs), c,
                                _norm_dtype(dtype, bufs), float(max_norm), float(eps), _ptr(stats),
                                _stream(stream, comm)), f"clip_multi ({algo})")
    return stats


def _loopback_norm(name: str, bufs, stats, counts):
    n = len(bufs[0])
    if any(len(b) != n for b in bufs) or len(stats) != len(bufs):
        raise ValueError(f"{name}: the ranks' lists differ in length")
    if counts is None:
        counts = [[b.numel() for b in r] for r in bufs]
    if len(counts) != len(bufs) or any(len(c) != n for c in counts):
        raise ValueError(f"{name}: counts and bufs differ in length")
    flat = [b for r in bufs for b in r]
    flat_c = [c for r in counts for c in r]
    return n, flat, (ctypes.c_size_t * max(len(flat_c), 1))(*flat_c)


def loopback_norm_multi(comms, algo, bufs, dtype, stats, counts=None):
    """bufs: one list of tensors per virtual rank; counts likewise (None: each
    tensor's numel()); stats: one device float64 buffer of n + 1 per rank.
    Returns (status, per-rank statuses)."""
    st = (ctypes.c_int * len(comms))()
    hs = (ctypes.c_void_p * len(comms))(*[c.handle.value for c in comms])
    n, flat, c = _loopback_norm("loopback_norm_multi", bufs, stats, counts)
    rc = lib().bine_loopback_run_norm_multi(hs, len(comms), _algo("allreduce", algo), n, _ptrs(flat), c,
                                            _norm_dtype(dtype, flat), _ptrs(stats), st)
    return rc, list(st)


def loopback_clip_multi(comms, algo, bufs, dtype, max_norm, eps, stats, counts=None, scale=True):
    """as loopback_norm_multi, clip_multi on every virtual rank; stats: n + 2
    float64 per rank.  scale=False as clip_multi's: the coefficient alone, each
    rank's clip_segments on its communicator's stream."""
    if not scale:
        _coef_only_args("loopback_clip_multi", max_norm, eps)
        rc, st = loopback_norm_multi(comms, algo, bufs, dtype, stats, counts=counts)
        if rc == 0 and not any(st):
            n, dt = len(bufs[0]), _norm_dtype(dtype, [b for r in bufs for b in r])
            for cm, s in zip(comms, stats):
                a = _ptr(s)
                clip_segments([], a + 8 * n, max_norm, eps, dtype=dt, counts=[], coef_out=a + 8 * (n + 1),
                              stream=cm.stream)
        return rc, st
    st = (ctypes.c_int * len(comms))()
    hs = (ctypes.c_void_p * len(comms))(*[c.handle.value for c in comms])
    n, flat, c = _loopback_norm("loopback_clip_multi", bufs, stats, counts)
    rc = lib().bine_loopback_run_clip_multi(hs, len(comms), _algo("allreduce", algo), n, _ptrs(flat), c,
                                            _norm_dtype(dtype, flat), float(max_norm), float(eps), _ptrs(stats), st)
    return rc, list(st)


# ---- fused AdamW step over a bucket of shards ----------------------------------------------

def adamw_consts(lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int):
    """The step's eight float32 constants (bine_adamw_consts, host only), each
    computed in float64 and rounded once: dk = 1 - lr * weight_decay, b1,
    1 - b1, b2, 1 - b2, rbc2 = 1 / sqrt(1 - b2^step), eps, ss = lr / (1 -
    b1^step).  Returns a numpy float32 array of 8."""
    import numpy as np
    out = (ctypes.c_float * 8)()
    check(lib().bine_adamw_consts(float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
                                  out), "bine_adamw_consts")
    return np.frombuffer(out, dtype=np.float32).copy()


def _adamw_dtype(dtype, bufs, default: str = "float") -> int:
    if isinstance(dtype, int):
        return dtype
    if dtype is None and not any(hasattr(b, "dtype") for b in (bufs or ())):
        dtype = default
    return _dtype(dtype, *(bufs or ()))


def plan_adamw(p: Sequence[int], m: Sequence[int], v: Sequence[int], g: Sequence[int], pout, counts: Sequence[int],
               gdtype, odtype="float"):
    """The launches of adamw_segments for these device addresses (pout None:
    no narrowed copy), element counts and types (bine_plan_adamw, host only):
    a list of (launch, segment, first workgroup in the launch, workgroups,
    body) per non-empty segment, body 0 = vector, 1 = element."""
    n = len(counts)
    if any(len(a) != n for a in (p, m, v, g)) or (pout is not None and len(pout) != n):
        raise ValueError("plan_adamw: the address lists and counts differ in length")
    arr = lambda a: (ctypes.c_uint64 * max(n, 1))(*a)  # noqa: E731
    args = (n, arr(p), arr(m), arr(v), arr(g), None if pout is None else arr(pout),
            (ctypes.c_size_t * max(n, 1))(*counts), _adamw_dtype(gdtype, ()), _adamw_dtype(odtype, ()))
    cap = lib().bine_plan_adamw(*args, None, 0)
    if cap < 0:
        raise BineError(int(-cap), "bine_plan_adamw")
    out = (ctypes.c_uint64 * (5 * max(cap, 1)))()
    lib().bine_plan_adamw(*args, out, cap)
    return [tuple(out[5 * t:5 * t + 5]) for t in range(cap)]


def _adamw_lists(name: str, p, m, v, g, pout, counts):
    n = len(p)
    if any(len(a) != n for a in (m, v, g)) or (pout is not None and len(pout) != n):
        raise ValueError(f"{name}: the tensor lists differ in length")
    return _norm_counts(name, p, counts)


def adamw_segments(p, m, v, g, pout=None, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999,
                   eps: float = 1e-8, weight_decay: float = 0.01, step: int = 1, gcoef=None, grad_mul: float = 1.0,
                   gdtype=None, odtype=None, counts=None, stream=None) -> None:
    """One fused AdamW step of every shard (bine_adamw_segments): p, m, v float32
    in place, g (float / float16 / bfloat16) read only, pout (optional, the same
    three types) = the new parameter narrowed.  gcoef: a device float64 that
    scales the gradient (clip_multi(..., scale=False)'s stats[n + 1:] -- after a
    clip that scaled g in place pass None), None = 1.0; grad_mul a
    host factor (1 / loss scale).  Per element, every line one float32
    operation: gs = g * float32(gcoef * grad_mul); p1 = p * dk; m = m * b1 +
    gs * (1 - b1); v = v * b2 + (gs * gs) * (1 - b2); d = sqrt(v) * rbc2 + eps;
    p = p1 - ss * (m / d), constants as adamw_consts.  Empty shards may be
    None; the tensors must not overlap."""
    c = _adamw_lists("adamw_segments", p, m, v, g, pout, counts)
    check(lib().bine_adamw_segments(len(p), _ptrs(p), _ptrs(m), _ptrs(v), _ptrs(g),
                                    None if pout is None else _ptrs(pout), c, _adamw_dtype(gdtype, g),
                                    _adamw_dtype(odtype, pout), float(lr), float(beta1), float(beta2), float(eps),
                                    float(weight_decay), int(step), _ptr(gcoef), float(grad_mul),
                                    _stream(stream, None)), "bine_adamw_segments")


def adamw_multi(ag_algo, params, p, m, v, g, comm: Comm, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999,
                eps: float = 1e-8, weight_decay: float = 0.01, step: int = 1, gcoef=None, grad_mul: float = 1.0,
                gdtype=None, odtype=None, shard_counts=None, stream=None) -> None:
    """bine_adamw_multi: adamw_segments with pout = this rank's slot of each full
    parameter tensor params[k] (comm.size * shard_counts[k] elements of odtype),
    then allgather_multi in place on params -- bit for bit those two calls."""
    c = _adamw_lists("adamw_multi", p, m, v, g, params, shard_counts)
    check(lib().bine_adamw_multi(comm.handle, _algo("allgather", ag_algo), len(p), _ptrs(params), _ptrs(p), _ptrs(m),
                                 _ptrs(v), _ptrs(g), c, _adamw_dtype(gdtype, g), _adamw_dtype(odtype, params),
                                 float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
                                 _ptr(gcoef), float(grad_mul), _stream(stream, comm)), f"adamw_multi ({ag_algo})")


def loopback_adamw_multi(comms, ag_algo, params, p, m, v, g, lr: float = 1e-3, beta1: float = 0.9,
                         beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.01, step: int = 1,
                         gcoef=None, grad_mul: float = 1.0, gdtype=None, odtype=None, shard_counts=None):
    """adamw_multi on every virtual rank: params, p, m, v, g one list of tensors
    per rank; shard_counts likewise (None: each p's numel()); gcoef one device
    float64 per rank, or None.  Returns (status, per-rank statuses)."""
    P = len(comms)
    n = len(p[0])
    if any(len(x) != P for x in (params, p, m, v, g)) or any(len(r) != n for x in (params, p, m, v, g) for r in x):
        raise ValueError("loopback_adamw_multi: the ranks' lists differ in length")
    if shard_counts is None:
        shard_counts = [[t.numel() for t in r] for r in p]
    flat = lambda x: [t for r in x for t in r]  # noqa: E731
    fc = flat(shard_counts)
    st = (ctypes.c_int * P)()
    hs = (ctypes.c_void_p * P)(*[c.handle.value for c in comms])
    rc = lib().bine_loopback_run_adamw_multi(
        hs, P, _algo("allgather", ag_algo), n, _ptrs(flat(params)), _ptrs(flat(p)), _ptrs(flat(m)), _ptrs(flat(v)),
        _ptrs(flat(g)), (ctypes.c_size_t * max(len(fc), 1))(*fc), _adamw_dtype(gdtype, flat(g)),
        _adamw_dtype(odtype, flat(params)), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
        int(step), None if gcoef is None else _ptrs(gcoef), float(grad_mul), st)
    return rc, list(st)


# ---- dynamic loss scaling: the step state and the skipping AdamW step ----------------------

STEP_STATE_FIELDS = ("scale", "good", "step", "pw1", "pw2", "skip", "gm", "skipped")


def _step_hyper(lr, beta1, beta2, eps, weight_decay, max_norm, clip_eps, growth_factor, backoff_factor,
                growth_interval, min_scale, max_scale):
    return _lib.StepHyper(float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), float(max_norm),
                          float(clip_eps), float(growth_factor), float(backoff_factor), float(min_scale),
                          float(max_scale), int(growth_interval))


def step_state_init(scale: float = 65536.0, step: int = 0, beta1: float = 0.9, beta2: float = 0.999):
    """A fresh step state (bine_step_state_init, host only): a numpy uint8 array of
    96 bytes -- eight float64 (scale, good, step, pw1, pw2, skip, gm, skipped) and
    eight float32 (the latest taken step's adamw_consts).  step > 0 resumes after
    that many taken steps: pw1 = beta1^step and pw2 = beta2^step as `step`
    sequential float64 multiplications.  Copy it to the device (any 8-byte
    aligned 96 bytes) for step_update / adamw_segments_dyn; saving and restoring
    a state is copying its bytes."""
    import numpy as np
    buf = np.zeros(_lib.STEP_STATE_BYTES // 8, dtype=np.float64)     # 8-byte aligned
    check(lib().bine_step_state_init(buf.ctypes.data, float(scale), int(step), float(beta1), float(beta2)),
          "bine_step_state_init")
    return buf.view(np.uint8)


def step_update_host(state, norm2: float, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999,
                     eps: float = 1e-8, weight_decay: float = 0.01, max_norm: float = float("inf"),
                     clip_eps: float = 1e-6, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                     growth_interval: int = 2000, min_scale: float = 1.0, max_scale: float = 2.0 ** 24) -> None:
    """step_update's host twin (bine_step_update_host): the same statement on a
    numpy state block (96 bytes, 8-byte aligned, updated in place) and a host
    float norm2."""
    h = _step_hyper(lr, beta1, beta2, eps, weight_decay, max_norm, clip_eps, growth_factor, backoff_factor,
                    growth_interval, min_scale, max_scale)
    if state.nbytes != _lib.STEP_STATE_BYTES or not state.flags["C_CONTIGUOUS"] or not state.flags["WRITEABLE"]:
        raise ValueError("step_update_host: state is not a writable block of 96 bytes")
    check(lib().bine_step_update_host(state.ctypes.data, float(norm2), ctypes.byref(h)), "bine_step_update_host")


def step_update(state, norm2, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                weight_decay: float = 0.01, max_norm: float = float("inf"), clip_eps: float = 1e-6,
                growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000,
                min_scale: float = 1.0, max_scale: float = 2.0 ** 24, stream=None) -> None:
    """The loss-scale and step-count update on the device (bine_step_update, one
    launch, stream-ordered, no host synchronization): `state` the 96-byte block
    in device memory, `norm2` a device float64 -- norm_multi's stats[n:], the
    squared norm of the SCALED gradient over all ranks.  norm2 infinite or NaN
    (some element on some rank overflowed): skip = 1, the scale backs off, the
    step count stays.  Otherwise the step counts, gm = min(1, max_norm /
    (sqrt(norm2) / scale + clip_eps)) / scale, the step's adamw_consts are
    formed from running products of the betas, and after growth_interval good
    updates the scale grows.  Every operation float64 (include/bine_amd.h)."""
    h = _step_hyper(lr, beta1, beta2, eps, weight_decay, max_norm, clip_eps, growth_factor, backoff_factor,
                    growth_interval, min_scale, max_scale)
    check(lib().bine_step_update(_ptr(state), _ptr(norm2), ctypes.byref(h), _stream(stream, None)),
          "bine_step_update")


def step_state_read(state) -> dict:
    """The state's fields as a dict: scale, good, step, pw1, pw2, skip, gm, skipped
    (Python floats) and consts (numpy float32 of 8).  A device tensor is copied
    to the host, which SYNCHRONIZES with its stream: for logging and
    checkpoints, not for the training loop."""
    import numpy as np
    if hasattr(state, "detach"):
        state = state.detach().contiguous().cpu().numpy()
    raw = np.ascontiguousarray(state).view(np.uint8).reshape(-1)
    if raw.size != _lib.STEP_STATE_BYTES:
        raise ValueError("step_state_read: state is not a block of 96 bytes")
    d = raw[:64].copy().view(np.float64)
    out = {k: float(x) for k, x in zip(STEP_STATE_FIELDS, d)}
    out["consts"] = raw[64:].copy().view(np.float32)
    return out


def adamw_segments_dyn(p, m, v, g, state, pout=None, gdtype=None, odtype=None, counts=None, stream=None) -> None:
    """adamw_segments with everything but the tensors read from the device
    state step_update left (bine_adamw_segments_dyn): skip != 0 stores nothing
    -- p, m, v and pout keep every bit -- otherwise gm = float32(state gm) and
    the state's eight constants.  No hyper-parameter, no step number and no
    decision on the host."""
    c = _adamw_lists("adamw_segments_dyn", p, m, v, g, pout, counts)
    check(lib().bine_adamw_segments_dyn(len(p), _ptrs(p), _ptrs(m), _ptrs(v), _ptrs(g),
                                        None if pout is None else _ptrs(pout), c, _adamw_dtype(gdtype, g),
                                        _adamw_dtype(odtype, pout), _ptr(state), _stream(stream, None)),
          "bine_adamw_segments_dyn")


def adamw_multi_dyn(ag_algo, params, p, m, v, g, state, comm: Comm, gdtype=None, odtype=None, shard_counts=None,
                    stream=None) -> None:
    """bine_adamw_multi_dyn: adamw_segments_dyn into this rank's slot of every
    params[k], then allgather_multi in place.  The allgather runs after a
    skipped step too (the host does not know) and gathers the slots as they
    stand, so params must hold the current parameters before the first call."""
    c = _adamw_lists("adamw_multi_dyn", p, m, v, g, params, shard_counts)
    check(lib().bine_adamw_multi_dyn(comm.handle, _algo("allgather", ag_algo), len(p), _ptrs(params), _ptrs(p),
                                     _ptrs(m), _ptrs(v), _ptrs(g), c, _adamw_dtype(gdtype, g),
                                     _adamw_dtype(odtype, params), _ptr(state), _stream(stream, comm)),
          f"adamw_multi_dyn ({ag_algo})")


def loopback_adamw_multi_dyn(comms, ag_algo, params, p, m, v, g, states, gdtype=None, odtype=None,
                             shard_counts=None):
    """adamw_multi_dyn on every virtual rank: lists as loopback_adamw_multi,
    states one device block per rank.  Returns (status, per-rank statuses)."""
    P = len(comms)
    n = len(p[0])
    if any(len(x) != P for x in (params, p, m, v, g, states)) or \
            any(len(r) != n for x in (params, p, m, v, g) for r in x):
        raise ValueError("loopback_adamw_multi_dyn: the ranks' lists differ in length")
    if shard_counts is None:
        shard_counts = [[t.numel() for t in r] for r in p]
    flat = lambda x: [t for r in x for t in r]  # noqa: E731
    fc = flat(shard_counts)
    st = (ctypes.c_int * P)()
    hs = (ctypes.c_void_p * P)(*[c.handle.value for c in comms])
    rc = lib().bine_loopback_run_adamw_multi_dyn(
        hs, P, _algo("allgather", ag_algo), n, _ptrs(flat(params)), _ptrs(flat(p)), _ptrs(flat(m)), _ptrs(flat(v)),
        _ptrs(flat(g)), (ctypes.c_size_t * max(len(fc), 1))(*fc), _adamw_dtype(gdtype, flat(g)),
        _adamw_dtype(odtype, flat(params)), _ptrs(states), st)
    return rc, list(st)


# ---- FP8 quantization of a bucket with per-tensor scaling -----------------------------------

def _fp8(fmt) -> int:
    return fmt if isinstance(fmt, int) else _lib.FP8_FORMATS[fmt]


def _dev_of(bufs):
    return next((b.device for b in bufs if hasattr(b, "device")), "cuda")


def amax_segments(bufs, dtype=None, counts=None, out=None, stream=None):
    """out[k] = the bit pattern of tensor k's largest |x| widened to float32
    (bine_amax_segments): the maximum of bits(x) & 0x7fffffff as unsigned
    integers, so any NaN shows as a pattern above infinity's and an empty tensor
    gives 0.  float / float16 / bfloat16; empty tensors may be None.  `out`: n
    int32 on the device holding the uint32 patterns (allocated when None).
    Returns out."""
    n = len(bufs)
    c = _norm_counts("amax_segments", bufs, counts)
    if out is None:
        import torch
        out = torch.empty(max(n, 1), dtype=torch.int32, device=_dev_of(bufs))
    check(lib().bine_amax_segments(n, _ptrs(bufs), c, _adamw_dtype(dtype, bufs), _ptr(out), _stream(stream, None)),
          "bine_amax_segments")
    return out


def fp8_scale_host(amax_bits: int, fmt):
    """(scale, inverse) for one amax pattern (bine_fp8_scale_host, host only):
    scale = 2^e with e the largest exponent for which amax * 2^e <= FMAX (448
    for "e4m3", 57344 for "e5m2"), clamped to [-126, 126]; e = 0 for an all-zero
    tensor and for inf / NaN."""
    s, i = ctypes.c_float(), ctypes.c_float()
    check(lib().bine_fp8_scale_host(int(amax_bits) & 0xFFFFFFFF, _fp8(fmt), ctypes.byref(s), ctypes.byref(i)),
          "bine_fp8_scale_host")
    return s.value, i.value


def fp8_scales(amax, fmt, n: int, scales=None, stream=None):
    """scales[k] = the scale of amax[k], scales[n + k] its inverse, on the device
    (bine_fp8_scales; the rule of fp8_scale_host).  amax: the n patterns
    amax_segments wrote (int32 tensor or address; n is the caller's, a tensor
    allocated for an empty list still has one word); scales: 2n float32
    (allocated when None).  Returns scales."""
    if scales is None:
        import torch
        scales = torch.empty(max(2 * n, 1), dtype=torch.float32, device=_dev_of([amax]))
    check(lib().bine_fp8_scales(n, _ptr(amax), _fp8(fmt), _ptr(scales), _stream(stream, None)), "bine_fp8_scales")
    return scales


def plan_quant(wide: Sequence[int], bytes8: Sequence[int], counts: Sequence[int], dtype):
    """The launches of quant_segments for these source (`wide`) and destination
    (`bytes8`) addresses -- of dequant_segments with the destination as `wide`
    -- (bine_plan_quant, host only): a list of (launch, segment, first workgroup
    in the launch, workgroups, body) per non-empty segment, body 0 = vector,
    1 = element."""
    n = len(counts)
    if len(wide) != n or len(bytes8) != n:
        raise ValueError("plan_quant: the address lists and counts differ in length")
    arr = lambda a: (ctypes.c_uint64 * max(n, 1))(*a)  # noqa: E731
    args = (n, arr(wide), arr(bytes8), (ctypes.c_size_t * max(n, 1))(*counts), _adamw_dtype(dtype, ()))
    cap = lib().bine_plan_quant(*args, None, 0)
    if cap < 0:
        raise BineError(int(-cap), "bine_plan_quant")
    out = (ctypes.c_uint64 * (5 * max(cap, 1)))()
    lib().bine_plan_quant(*args, out, cap)
    return [tuple(out[5 * t:5 * t + 5]) for t in range(cap)]


def quant_segments(src, dst8, fmt, scales=None, sdtype=None, counts=None, stream=None) -> None:
    """dst8[k] = tensor src[k] times scales[k] in OCP FP8, one byte per element
    (bine_quant_segments): one float32 multiplication, NaN -> 0x7F, everything
    else clamped to +-FMAX and rounded to nearest even.  src float / float16 /
    bfloat16; dst8 uint8 at any byte alignment; scales: n float32 on the device
    (fp8_scales' first half), None = 1.  Empty tensors may be None."""
    if len(src) != len(dst8):
        raise ValueError("quant_segments: src and dst8 differ in length")
    c = _norm_counts("quant_segments", src, counts)
    check(lib().bine_quant_segments(len(src), _ptrs(src), _ptrs(dst8), c, _adamw_dtype(sdtype, src), _fp8(fmt),
                                    _ptr(scales), _stream(stream, None)), "bine_quant_segments")


def dequant_segments(src8, dst, fmt, inv_scales=None, ddtype=None, counts=None, stream=None) -> None:
    """dst[k] = the FP8 bytes src8[k] decoded exactly, times inv_scales[k] in
    float32, rounded once into dst's type (bine_dequant_segments).  inv_scales:
    n float32 on the device (fp8_scales' second half), None = 1."""
    if len(src8) != len(dst):
        raise ValueError("dequant_segments: src8 and dst differ in length")
    c = _norm_counts("dequant_segments", dst, counts)
    check(lib().bine_dequant_segments(len(dst), _ptrs(src8), _ptrs(dst), c, _adamw_dtype(ddtype, dst), _fp8(fmt),
                                      _ptr(inv_scales), _stream(stream, None)), "bine_dequant_segments")


def quant_multi(amax_algo, ag_algo, params8, src, fmt, comm: Comm, scales=None, sdtype=None, shard_counts=None,
                stream=None):
    """bine_quant_multi: this rank's shards src[k] quantized with one scale per
    tensor agreed over all ranks, and the bytes gathered into params8[k]
    (comm.size * shard_counts[k] uint8) -- bit for bit amax_segments, one
    in-place allreduce (uint32, max) of the patterns, fp8_scales, quant_segments
    into this rank's slots, allgather_multi in place as uint8.  scales: 2n
    float32 on the device (allocated when None), the same bits on every rank.
    Returns scales."""
    if len(params8) != len(src):
        raise ValueError("quant_multi: params8 and src differ in length")
    n = len(src)
    c = _norm_counts("quant_multi", src, shard_counts)
    if scales is None:
        import torch
        scales = torch.empty(max(2 * n, 1), dtype=torch.float32, device=_dev_of(src))
    check(lib().bine_quant_multi(comm.handle, _algo("allreduce", amax_algo), _algo("allgather", ag_algo), n,
                                 _ptrs(params8), _ptrs(src), c, _adamw_dtype(sdtype, src), _fp8(fmt), _ptr(scales),
                                 _stream(stream, comm)), f"quant_multi ({amax_algo}, {ag_algo})")
    return scales


def loopback_quant_multi(comms, amax_algo, ag_algo, params8, src, fmt, scales, sdtype=None, shard_counts=None):
    """quant_multi on every virtual rank: params8 and src one list of tensors
    per rank, shard_counts one list for all ranks (None: rank 0's numel()),
    scales one device float32 buffer of 2n per rank.  Returns (status, per-rank
    statuses)."""
    P = len(comms)
    n = len(src[0])
    if any(len(x) != P for x in (params8, src, scales)) or any(len(r) != n for x in (params8, src) for r in x):
        raise ValueError("loopback_quant_multi: the ranks' lists differ in length")
    if shard_counts is None:
        shard_counts = [t.numel() for t in src[0]]
    flat = lambda x: [t for r in x for t in r]  # noqa: E731
    st = (ctypes.c_int * P)()
    hs = (ctypes.c_void_p * P)(*[c.handle.value for c in comms])
    rc = lib().bine_loopback_run_quant_multi(
        hs, P, _algo("allreduce", amax_algo), _algo("allgather", ag_algo), n, _ptrs(flat(params8)), _ptrs(flat(src)),
        (ctypes.c_size_t * max(n, 1))(*shard_counts), _adamw_dtype(sdtype, flat(src)), _fp8(fmt), _ptrs(scales), st)
    return rc, list(st)


# ---- MX block-scaled quantization of a bucket (32 elements per E8M0 scale byte) -------------

def _mx(fmt) -> int:
    return fmt if isinstance(fmt, int) else _lib.MX_FORMATS[fmt]


def mx_dbytes(count: int, fmt) -> int:
    """The data bytes of `count` elements: one each, two per byte for "e2m1"."""
    return (count + 1) // 2 if _mx(fmt) == _lib.MX_FORMATS["e2m1"] else count


def mx_scale_host(amax_bits: int, fmt) -> int:
    """The E8M0 scale byte of a block whose largest bits(x) & 0x7fffffff is
    amax_bits (bine_mx_scale_host, host only): 0xFF for an inf or a NaN, 0 for
    an all-zero block, else max(floor(log2 amax) - emax + 127, 0) with emax 8
    ("e4m3"), 15 ("e5m2") or 2 ("e2m1")."""
    s = ctypes.c_uint8()
    check(lib().bine_mx_scale_host(int(amax_bits) & 0xFFFFFFFF, _mx(fmt), ctypes.byref(s)), "bine_mx_scale_host")
    return s.value


def plan_mx(wide: Sequence[int], data8: Sequence[int], scl8: Sequence[int], counts: Sequence[int], dtype, fmt):
    """The launches of mx_quant_segments for these source (`wide`), data and
    scale addresses -- of mx_dequant_segments with the destination as `wide` --
    (bine_plan_mx, host only): a list of (launch, segment, first workgroup in
    the launch, workgroups, body) per non-empty segment, body 0 = vector,
    1 = element."""
    n = len(counts)
    if len(wide) != n or len(data8) != n or len(scl8) != n:
        raise ValueError("plan_mx: the address lists and counts differ in length")
    arr = lambda a: (ctypes.c_uint64 * max(n, 1))(*a)  # noqa: E731
    args = (n, arr(wide), arr(data8), arr(scl8), (ctypes.c_size_t * max(n, 1))(*counts), _adamw_dtype(dtype, ()),
            _mx(fmt))
    cap = lib().bine_plan_mx(*args, None, 0)
    if cap < 0:
        raise BineError(int(-cap), "bine_plan_mx")
    out = (ctypes.c_uint64 * (5 * max(cap, 1)))()
    lib().bine_plan_mx(*args, out, cap)
    return [tuple(out[5 * t:5 * t + 5]) for t in range(cap)]


def mx_quant_segments(src, dst8, scl8, fmt, sdtype=None, counts=None, stream=None) -> None:
    """Tensor src[k] as OCP MX blocks (bine_mx_quant_segments): every 32
    elements, counted from the tensor's first, share the scale byte scl8[k][b]
    = mx_scale_host of the block's largest magnitude, and dst8[k] holds
    widen(x) * 2^(127 - S) clamped to +-FMAX and rounded to nearest even into
    "e4m3" / "e5m2" (one byte each) or "e2m1" (two per byte, the even element
    in the low nibble).  A block with an inf or a NaN gets S = 0xFF and zero
    data.  src float / float16 / bfloat16; dst8 and scl8 uint8 at any byte
    alignment, mx_dbytes(count) and ceil(count / 32) bytes.  Empty tensors may
    be None."""
    if len(src) != len(dst8) or len(src) != len(scl8):
        raise ValueError("mx_quant_segments: src, dst8 and scl8 differ in length")
    c = _norm_counts("mx_quant_segments", src, counts)
    check(lib().bine_mx_quant_segments(len(src), _ptrs(src), _ptrs(dst8), _ptrs(scl8), c, _adamw_dtype(sdtype, src),
                                       _mx(fmt), _stream(stream, None)), "bine_mx_quant_segments")


def mx_dequant_segments(src8, scl8, dst, fmt, ddtype=None, counts=None, stream=None) -> None:
    """dst[k] = the MX data src8[k] decoded exactly, times 2^(S - 127) of its
    block's scale byte in float32, rounded once into dst's type
    (bine_mx_dequant_segments); S = 0xFF gives quiet NaNs."""
    if len(src8) != len(dst) or len(scl8) != len(dst):
        raise ValueError("mx_dequant_segments: src8, scl8 and dst differ in length")
    c = _norm_counts("mx_dequant_segments", dst, counts)
    check(lib().bine_mx_dequant_segments(len(dst), _ptrs(src8), _ptrs(scl8), _ptrs(dst), c, _adamw_dtype(ddtype, dst),
                                         _mx(fmt), _stream(stream, None)), "bine_mx_dequant_segments")


def mx_quant_multi(ag_algo, params8, scales8, src, fmt, comm: Comm, sdtype=None, shard_counts=None, stream=None):
    """bine_mx_quant_multi: this rank's shards src[k] quantized into its slots
    of params8[k] (comm.size * mx_dbytes(shard_counts[k]) uint8) and scales8[k]
    (comm.size * shard_counts[k] / 32 uint8), then ONE in-place allgather_multi
    over the 2n buffers as uint8.  Every shard count a multiple of 32."""
    if len(params8) != len(src) or len(scales8) != len(src):
        raise ValueError("mx_quant_multi: params8, scales8 and src differ in length")
    c = _norm_counts("mx_quant_multi", src, shard_counts)
    check(lib().bine_mx_quant_multi(comm.handle, _algo("allgather", ag_algo), len(src), _ptrs(params8),
                                    _ptrs(scales8), _ptrs(src), c, _adamw_dtype(sdtype, src), _mx(fmt),
                                    _stream(stream, comm)), f"mx_quant_multi ({ag_algo})")


def loopback_mx_quant_multi(comms, ag_algo, params8, scales8, src, fmt, sdtype=None, shard_counts=None):
    """mx_quant_multi on every virtual rank: params8, scales8 and src one list
    of tensors per rank, shard_counts one list for all ranks (None: rank 0's
    numel()).  Returns (status, per-rank statuses)."""
    P = len(comms)
    n = len(src[0])
    if any(len(x) != P for x in (params8, scales8, src)) or \
            any(len(r) != n for x in (params8, scales8, src) for r in x):
        raise ValueError("loopback_mx_quant_multi: the ranks' lists differ in length")
    if shard_counts is None:
        shard_counts = [t.numel() for t in src[0]]
    flat = lambda x: [t for r in x for t in r]  # noqa: E731
    st = (ctypes.c_int * P)()
    hs = (ctypes.c_void_p * P)(*[c.handle.value for c in comms])
    rc = lib().bine_loopback_run_mx_quant_multi(
        hs, P, _algo("allgather", ag_algo), n, _ptrs(flat(params8)), _ptrs(flat(scales8)), _ptrs(flat(src)),
        (ctypes.c_size_t * max(n, 1))(*shard_counts), _adamw_dtype(sdtype, flat(src)), _mx(fmt), st)
    return rc, list(st)


# ---- MX-quantized gradient reduce-scatter of a bucket ----------------------------------------

def mx_wire_bytes(shard_counts: Sequence[int], fmt):
    """(D, B) of a bucket's wire block (bine_mx_wire_bytes, host only): D data
    bytes -- tensor k's at the prefix sum of mx_dbytes before k -- then the
    scale bytes, one per 32 elements in tensor order, B = D + S rounded up to a
    multiple of 16.  Every count a multiple of 32."""
    n = len(shard_counts)
    d, b = ctypes.c_size_t(), ctypes.c_size_t()
    check(lib().bine_mx_wire_bytes(n, (ctypes.c_size_t * max(n, 1))(*shard_counts), _mx(fmt), ctypes.byref(d),
                                   ctypes.byref(b)), "bine_mx_wire_bytes")
    return d.value, b.value


def plan_mx_sum(dst: Sequence[int], counts: Sequence[int], ddtype, fmt):
    """The launches of mx_sum_segments for these destination addresses
    (bine_plan_mx_sum, host only): plan_mx's records, body 0 = vector (dst
    16-B aligned), 1 = element."""
    n = len(counts)
    if len(dst) != n:
        raise ValueError("plan_mx_sum: dst and counts differ in length")
    args = (n, (ctypes.c_uint64 * max(n, 1))(*dst), (ctypes.c_size_t * max(n, 1))(*counts), _adamw_dtype(ddtype, ()),
            _mx(fmt))
    cap = lib().bine_plan_mx_sum(*args, None, 0)
    if cap < 0:
        raise BineError(int(-cap), "bine_plan_mx_sum")
    out = (ctypes.c_uint64 * (5 * max(cap, 1)))()
    lib().bine_plan_mx_sum(*args, out, cap)
    return [tuple(out[5 * t:5 * t + 5]) for t in range(cap)]


def mx_sum_segments(packed, nstreams: int, block_bytes: int, dst, fmt, scale: float = 1.0, ddtype=None, counts=None,
                    stream=None) -> None:
    """dst[k][i] = narrow((d_0 + d_1 + ... in that order, float32) * scale) over
    the nstreams (1 .. 16) wire blocks of `packed`, block j at packed + j *
    block_bytes in mx_wire_bytes' layout, d_j = decode(data) * 2^(S - 127)
    exactly (bine_mx_sum_segments).  A block of 32 whose scale byte is 0xFF in
    any stream gives quiet NaNs.  packed: uint8, 16-B aligned."""
    c = _norm_counts("mx_sum_segments", dst, counts)
    check(lib().bine_mx_sum_segments(len(dst), int(nstreams), _ptr(packed), int(block_bytes), _ptrs(dst), c,
                                     _adamw_dtype(ddtype, dst), _mx(fmt), float(scale), _stream(stream, None)),
          "bine_mx_sum_segments")


def _mx_rs_scale(op: str, scale, comm: Comm) -> float:
    op, scale = _scaled(op, scale, comm)
    if op != "sum":
        raise ValueError('mx_reduce_scatter_multi: op is "sum" or "avg"')
    return 1.0 if scale is None else float(scale)


def mx_reduce_scatter_multi(sbufs, rbufs, fmt, comm: Comm, op: str = "sum", scale=None, a2a_algo="bine", sdtype=None,
                            rdtype=None, shard_counts=None, send_ws=None, recv_ws=None, stream=None):
    """bine_mx_reduce_scatter_multi: sbufs[k] holds comm.size shards of
    shard_counts[k] elements (float / float16 / bfloat16), rbufs[k] receives
    this rank's shard of their sum -- every shard quantized once to MX blocks
    (this rank's own too), ONE alltoall of comm.size blocks of mx_wire_bytes'
    B bytes, then mx_sum_segments: the contributions decoded and added in rank
    order in float32, times scale (op="avg": 1 / comm.size), rounded once into
    rbufs' type.  Every shard count a multiple of 32; rbufs[k] may overlap
    sbufs[k].  send_ws / recv_ws: comm.size * B uint8 each, 16-B aligned
    (allocated when None).  Returns (send_ws, recv_ws)."""
    if sbufs is None or len(sbufs) != len(rbufs):
        raise ValueError("mx_reduce_scatter_multi: sbufs and rbufs differ in length")
    s = _mx_rs_scale(op, scale, comm)
    if shard_counts is None:
        shard_counts = [b.numel() for b in rbufs]
    c = _norm_counts("mx_reduce_scatter_multi", rbufs, shard_counts)
    need = comm.size * mx_wire_bytes(list(shard_counts), fmt)[1]
    if send_ws is None or recv_ws is None:
        import torch
        dev = _dev_of(list(rbufs) + list(sbufs))
        send_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev) if send_ws is None else send_ws
        recv_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev) if recv_ws is None else recv_ws
    ws_bytes = min(send_ws.numel(), recv_ws.numel()) if hasattr(send_ws, "numel") and hasattr(recv_ws, "numel") else need
    check(lib().bine_mx_reduce_scatter_multi(comm.handle, _algo("alltoall", a2a_algo), len(rbufs), _ptrs(sbufs),
                                             _ptrs(rbufs), c, _adamw_dtype(sdtype, sbufs), _adamw_dtype(rdtype, rbufs),
                                             _mx(fmt), s, _ptr(send_ws), _ptr(recv_ws), ws_bytes,
                                             _stream(stream, comm)), f"mx_reduce_scatter_multi ({a2a_algo})")
    return send_ws, recv_ws


def loopback_mx_reduce_scatter_multi(comms, sbufs, rbufs, fmt, op: str = "sum", scale=None, a2a_algo="bine",
                                     sdtype=None, rdtype=None, shard_counts=None, send_ws=None, recv_ws=None):
    """mx_reduce_scatter_multi on every virtual rank: sbufs and rbufs one list
    of tensors per rank, shard_counts one list for all ranks (None: rank 0's
    rbufs' numel()), send_ws / recv_ws one uint8 buffer per rank (allocated
    when None).  Returns (status, per-rank statuses)."""
    P = len(comms)
    n = len(rbufs[0])
    if any(len(x) != P for x in (sbufs, rbufs)) or any(len(r) != n for x in (sbufs, rbufs) for r in x):
        raise ValueError("loopback_mx_reduce_scatter_multi: the ranks' lists differ in length")
    s = _mx_rs_scale(op, scale, comms[0])
    if shard_counts is None:
        shard_counts = [t.numel() for t in rbufs[0]]
    need = P * mx_wire_bytes(list(shard_counts), fmt)[1]
    flat = lambda x: [t for r in x for t in r]  # noqa: E731
    if send_ws is None or recv_ws is None:
        import torch
        dev = _dev_of(flat(rbufs) + flat(sbufs))
        mk = lambda: [torch.empty(max(need, 16), dtype=torch.uint8, device=dev) for _ in range(P)]  # noqa: E731
        send_ws = mk() if send_ws is None else send_ws
        recv_ws = mk() if recv_ws is None else recv_ws
    ws = [w.numel() for w in list(send_ws) + list(recv_ws) if hasattr(w, "numel")]
    ws_bytes = min(ws) if ws else need
    st = (ctypes.c_int * P)()
    hs = (ctypes.c_void_p * P)(*[c.handle.value for c in comms])
    rc = lib().bine_loopback_run_mx_reduce_scatter_multi(
        hs, P, _algo("alltoall", a2a_algo), n, _ptrs(flat(sbufs)), _ptrs(flat(rbufs)),
        (ctypes.c_size_t * max(n, 1))(*shard_counts), _adamw_dtype(sdtype, flat(sbufs)),
        _adamw_dtype(rdtype, flat(rbufs)), _mx(fmt), s, _ptrs(send_ws), _ptrs(recv_ws), ws_bytes, st)
    return rc, list(st)


# ---- the same with an error-feedback residual -------------------------------------------------

def plan_mx_ef(src: Sequence[int], res: Sequence[int], data8: Sequence[int], scl8: Sequence[int],
               counts: Sequence[int], dtype, fmt):
    """The launches of mx_quant_ef_segments for these source, residual, data
    and scale addresses (bine_plan_mx_ef, host only): plan_mx's records, at most
    MX_EF_SEGS_PER_LAUNCH segments per launch, body 0 = vector (source and
    residual 16-B aligned, data8 as plan_mx asks), 1 = element."""
    n = len(counts)
    if len(src) != n or len(res) != n or len(data8) != n or len(scl8) != n:
        raise ValueError("plan_mx_ef: the address lists and counts differ in length")
    arr = lambda a: (ctypes.c_uint64 * max(n, 1))(*a)  # noqa: E731
    args = (n, arr(src), arr(res), arr(data8), arr(scl8), (ctypes.c_size_t * max(n, 1))(*counts),
            _adamw_dtype(dtype, ()), _mx(fmt))
    cap = lib().bine_plan_mx_ef(*args, None, 0)
    if cap < 0:
        raise BineError(int(-cap), "bine_plan_mx_ef")
    out = (ctypes.c_uint64 * (5 * max(cap, 1)))()
    lib().bine_plan_mx_ef(*args, out, cap)
    return [tuple(out[5 * t:5 * t + 5]) for t in range(cap)]


def mx_quant_ef_segments(src, res, dst8, scl8, fmt, sdtype=None, counts=None, stream=None) -> None:
    """mx_quant_segments with an error-feedback residual
    (bine_mx_quant_ef_segments): v = widen(src) + res in float32 is what gets
    quantized -- scale bytes from v's blocks, data as mx_quant_segments gives
    for v -- and res is overwritten with v - decode * 2^(S - 127), exactly what
    the format dropped.  A block with an inf or a NaN in v gets S = 0xFF, zero
    data and zero residuals.  res[k]: float32, one per element of src[k]."""
    if len(src) != len(res) or len(src) != len(dst8) or len(src) != len(scl8):
        raise ValueError("mx_quant_ef_segments: src, res, dst8 and scl8 differ in length")
    c = _norm_counts("mx_quant_ef_segments", src, counts)
    check(lib().bine_mx_quant_ef_segments(len(src), _ptrs(src), _ptrs(res), _ptrs(dst8), _ptrs(scl8), c,
                                          _adamw_dtype(sdtype, src), _mx(fmt), _stream(stream, None)),
          "bine_mx_quant_ef_segments")


def mx_reduce_scatter_multi_ef(sbufs, res, rbufs, fmt, comm: Comm, op: str = "sum", scale=None, a2a_algo="bine",
                               sdtype=None, rdtype=None, shard_counts=None, send_ws=None, recv_ws=None, stream=None):
    """bine_mx_reduce_scatter_multi_ef: mx_reduce_scatter_multi whose first step
    is mx_quant_ef_segments.  res[k]: float32, comm.size * shard_counts[k]
    values laid out as sbufs[k], read and overwritten -- what this rank could
    not send now it adds to its contribution in the next call.  rbufs[k] may
    overlap sbufs[k] but not res[k].  Returns (send_ws, recv_ws)."""
    if sbufs is None or res is None or len(sbufs) != len(rbufs) or len(res) != len(rbufs):
        raise ValueError("mx_reduce_scatter_multi_ef: sbufs, res and rbufs differ in length")
    s = _mx_rs_scale(op, scale, comm)
    if shard_counts is None:
        shard_counts = [b.numel() for b in rbufs]
    c = _norm_counts("mx_reduce_scatter_multi_ef", rbufs, shard_counts)
    need = comm.size * mx_wire_bytes(list(shard_counts), fmt)[1]
    if send_ws is None or recv_ws is None:
        import torch
        dev = _dev_of(list(rbufs) + list(sbufs))
        send_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev) if send_ws is None else send_ws
        recv_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev) if recv_ws is None else recv_ws
    ws_bytes = min(send_ws.numel(), recv_ws.numel()) if hasattr(send_ws, "numel") and hasattr(recv_ws, "numel") else need
    check(lib().bine_mx_reduce_scatter_multi_ef(comm.handle, _algo("alltoall", a2a_algo), len(rbufs), _ptrs(sbufs),
                                                _ptrs(res), _ptrs(rbufs), c, _adamw_dtype(sdtype, sbufs),
                                                _adamw_dtype(rdtype, rbufs), _mx(fmt), s, _ptr(send_ws), _ptr(recv_ws),
                                                ws_bytes, _stream(stream, comm)),
          f"mx_reduce_scatter_multi_ef ({a2a_algo})")
    return send_ws, recv_ws


def loopback_mx_reduce_scatter_multi_ef(comms, sbufs, res, rbufs, fmt, op: str = "sum", scale=None, a2a_algo="bine",
                                        sdtype=None, rdtype=None, shard_counts=None, send_ws=None, recv_ws=None):
    """mx_reduce_scatter_multi_ef on every virtual rank: sbufs, res and rbufs
    one list of tensors per rank, the rest as loopback_mx_reduce_scatter_multi.
    Returns (status, per-rank statuses)."""
    P = len(comms)
    n = len(rbufs[0])
    if any(len(x) != P for x in (sbufs, res, rbufs)) or any(len(r) != n for x in (sbufs, res, rbufs) for r in x):
        raise ValueError("loopback_mx_reduce_scatter_multi_ef: the ranks' lists differ in length")
    s = _mx_rs_scale(op, scale, comms[0])
    if shard_counts is None:
        shard_counts = [t.numel() for t in rbufs[0]]
    need = P * mx_wire_bytes(list(shard_counts), fmt)[1]
    flat = lambda x: [t for r in x for t in r]  # noqa: E731
    if send_ws is None or recv_ws is None:
        import torch
        dev = _dev_of(flat(rbufs) + flat(sbufs))
        mk = lambda: [torch.empty(max(need, 16), dtype=torch.uint8, device=dev) for _ in range(P)]  # noqa: E731
        send_ws = mk() if send_ws is None else send_ws
        recv_ws = mk() if recv_ws is None else recv_ws
    ws = [w.numel() for w in list(send_ws) + list(recv_ws) if hasattr(w, "numel")]
    ws_bytes = min(ws) if ws else need
    st = (ctypes.c_int * P)()
    hs = (ctypes.c_void_p * P)(*[c.handle.value for c in comms])
    rc = lib().bine_loopback_run_mx_reduce_scatter_multi_ef(
        hs, P, _algo("alltoall", a2a_algo), n, _ptrs(flat(sbufs)), _ptrs(flat(res)), _ptrs(flat(rbufs)),
        (ctypes.c_size_t * max(n, 1))(*shard_counts), _adamw_dtype(sdtype, flat(sbufs)),
        _adamw_dtype(rdtype, flat(rbufs)), _mx(fmt), s, _ptrs(send_ws), _ptrs(recv_ws), ws_bytes, st)
    return rc, list(st)


def allreduce_staged(algo, host_sbuf, host_rbuf, dev_sbuf, dev_rbuf, count: int, dtype, op: str, comm: Comm,
                     h2d_stream, d2h_stream, segsize: int = 0, chunk_bytes: int = 0, stream=None) -> None:
    """bine_allreduce_staged: host buffers (page-locked) staged through the
    device buffers piece by piece, pipelined with the collective; synchronize
    `stream` to complete the call."""
    check(lib().bine_allreduce_staged(comm.handle, _algo("allreduce", algo), _ptr(host_sbuf), _ptr(host_rbuf),
                                      _ptr(dev_sbuf), _ptr(dev_rbuf), count, _dtype(dtype, dev_rbuf), OPS[op],
                                      segsize, chunk_bytes, _stream(h2d_stream, comm), _stream(d2h_stream, comm),
                                      _stream(stream, comm)), f"allreduce_staged_{algo}")


def reduce_scatter_staged(algo, host_sbuf, host_rbuf, dev_sbuf, dev_rbuf, rcounts: Sequence[int], dtype, op: str,
                          comm: Comm, h2d_stream, d2h_stream, chunk_bytes: int = 0, stream=None) -> None:
    """bine_reduce_scatter_staged (see allreduce_staged)."""
    rc = (ctypes.c_int * len(rcounts))(*rcounts)
    check(lib().bine_reduce_scatter_staged(comm.handle, _algo("reduce_scatter", algo), _ptr(host_sbuf),
                                           _ptr(host_rbuf), _ptr(dev_sbuf), _ptr(dev_rbuf), rc,
                                           _dtype(dtype, dev_rbuf), OPS[op], chunk_bytes,
                                           _stream(h2d_stream, comm), _stream(d2h_stream, comm),
                                           _stream(stream, comm)), f"reduce_scatter_staged_{algo}")


def reduce(algo, sbuf, rbuf, count: int, dtype, op: str, root: int, comm: Comm, stream=None) -> None:
    check(lib().bine_reduce(comm.handle, _algo("reduce", algo), _ptr(sbuf), _ptr(rbuf), count,
                            _dtype(dtype, sbuf if rbuf is None else rbuf), OPS[op], root, _stream(stream, comm)),
          f"reduce_{algo}")


# ---- loopback group drivers (all virtual ranks of one device) -------------------

def _ptrs(bufs):
    return (ctypes.c_void_p * len(bufs))(*[_ptr(b) for b in bufs])


def loopback_allreduce(comms, algo, sbufs, rbufs, count, dtype, op="sum", segsize=0, scale=None):
    st = (ctypes.c_int * len(comms))()
    hs = (ctypes.c_void_p * len(comms))(*[c.handle.value for c in comms])
    op, scale = _scaled(op, scale, comms[0])
    if scale is not None:
        rc = lib().bine_loopback_run_allreduce_scaled(hs, len(comms), _algo("allreduce", algo), _ptrs(sbufs),
                                                      _ptrs(rbufs), count, _dtype(dtype, rbufs[0]), OPS[op],
                                                      float(scale), segsize, st)
        return rc, list(st)
    rc = lib().bine_loopback_run_allreduce(hs, len(comms), _algo("allreduce", algo), _ptrs(sbufs), _ptrs(rbufs),
                                           count, _dtype(dtype, rbufs[0]), OPS[op], segsize, st)
    return rc, list(st)


def loopback_reduce_scatter(comms, algo, sbufs, rbufs, rcounts, dtype, op="sum", scale=None):
    st = (ctypes.c_int * len(comms))()
    hs = (ctypes.c_void_p * len(comms))(*[c.handle.value for c in comms])
    rcs = (ctypes.c_int * len(rcounts))(*rcounts)
    op, scale = _scaled(op, scale, comms[0])
    if scale is not None:
        rc = lib().bine_loopback_run_reduce_scatter_scaled(hs, len(comms), _algo("reduce_scatter", algo),
                                                           _ptrs(sbufs), _ptrs(rbufs), rcs,
                                                           _dtype(dtype, rbufs[0]), OPS[op], float(scale), st)
        return rc, list(st)
    rc = lib().bine_loopback_run_reduce_scatter(hs, len(comms), _algo("reduce_scatter", algo), _ptrs(sbufs),
                                                _ptrs(rbufs), rcs, _dtype(dtype, rbufs[0]), OPS[op], st)
    return rc, list(st)


def loopback_reduce(comms, algo, sbufs, rbufs, count, dtype, op="sum", root=0):
    st = (ctypes.c_int * len(comms))()
    hs = (ctypes.c_void_p * len(comms))(*[c.handle.value for c in comms])
    rc = lib().bine_loopback_run_reduce(hs, len(comms), _algo("reduce", algo), _ptrs(sbufs), _ptrs(rbufs),
                                        count, _dtype(dtype, sbufs[0]), OPS[op], root, st)
    return rc, list(st)


# ---- schedule introspection ------------------------------------------------------

def plan(coll: str, algo, nranks: int, rank: int, count: int = 0, rcounts=None, root: int = 0,
         esz: int = 4, segsize: int = 0, in_place: bool = False):
    """Rank `rank`'s primitive list (host only).  Returns (prims, tmp_elems) or
    raises BineError with the reference's error status."""
    a = _algo(coll, algo)
    rc = (ctypes.c_int * nranks)(*(rcounts or [0] * nranks))
    tmp = (ctypes.c_uint64 * 3)()
    n = lib().bine_plan(a, nranks, rank, count, rc, root, esz, segsize, int(in_place), None, 0, tmp)
    if n < 0:
        raise BineError(int(-n), f"plan {coll}_{algo}")
    arr = (_lib.Prim * max(int(n), 1))()
    lib().bine_plan(a, nranks, rank, count, rc, root, esz, segsize, int(in_place), arr, n, tmp)
    prims = [{f: getattr(arr[k], f) for f, _ in _lib.Prim._fields_ } for k in range(int(n))]
    for p in prims:
        p["type"] = _lib.PRIM_NAMES[p["type"]]
    return prims, list(tmp)


def schedule(coll: str, algo, nranks: int, rank: int, count: int = 0, rcounts=None, root: int = 0,
             esz: int = 4, segsize: int = 0, in_place: bool = False, chunk_bytes: int = 0,
             relay_min_bytes: int = 0, info: bool = False, trees: bool = False, flat_ag: bool = False,
             flat_rs: bool = False, scaled: bool = False, wide: bool = False):
    """The executor's two-stream issue schedule of rank `rank` (host only).
    scaled=True: of the scaled call (flagged trees, flags & PRIM_SCALED, or one
    trailing "SCALE").  wide=True (esz=2): of a path-B wide call (its final
    trees carry flags & PRIM_WIDE); a path-A call raises ERR_UNSUPPORTED.
    Returns (ops, c_join, final_wait); ops[i] = {"xchg", "wait", "prims"}.
    With info=True a 4th item: {"tmp_elems": [TMP0..2], "stage_elems": relay staging}."""
    a = _algo(coll, algo)
    rc = (ctypes.c_int * nranks)(*(rcounts or [0] * nranks))
    cj, fw, ws = ctypes.c_int(), ctypes.c_int64(), (ctypes.c_uint64 * 4)()
    args = (a, nranks, rank, count, rc, root, esz, segsize, int(in_place), chunk_bytes, relay_min_bytes,
            int(trees) | (2 if flat_ag else 0) | (4 if flat_rs else 0) | (8 if flat_ag == 2 else 0) |
            (16 if scaled else 0) | (32 if wide else 0))
    n = lib().bine_plan_schedule(*args, None, 0, ctypes.byref(cj), ctypes.byref(fw), ws)
    if n < 0:
        raise BineError(int(-n), f"schedule {coll}_{algo}")
    arr = (_lib.SchedEntry * max(int(n), 1))()
    lib().bine_plan_schedule(*args, arr, n, ctypes.byref(cj), ctypes.byref(fw), ws)
    ops = []
    for k in range(int(n)):
        e = arr[k]
        p = {f: getattr(e.prim, f) for f, _ in _lib.Prim._fields_ }
        p["type"] = _lib.PRIM_NAMES[p["type"]]
        if not ops or e.op != len(ops) - 1:
            ops.append({"xchg": bool(e.xchg), "wait": int(e.wait), "prims": []})
        ops[-1]["prims"].append(p)
    if info:
        return ops, bool(cj.value), int(fw.value), {"tmp_elems": [int(x) for x in ws[:3]],
                                                     "stage_elems": int(ws[3])}
    return ops, bool(cj.value), int(fw.value)


def dm_tree_plan(coll: str, algo, nranks: int, rank: int, count: int = 0, rcounts=None, esz: int = 4,
                 in_place: bool = False, chunk_bytes: int = 0, flat_ag=False, flat_rs: bool = False,
                 slot: int = 16 << 20, merge: int = 3, dtype="float", op: str = "sum"):
    """The direct transport's fused-tree decisions for rank `rank`'s issue
    schedule (bine_plan_dm_trees, host only): (host, defer) per op -- host[i]
    = the exchange whose launch evaluates tree op i (-1: not fused), defer[i]
    = exchange i's receives are pulled by the next exchange."""
    a = _algo(coll, algo)
    rc = (ctypes.c_int * nranks)(*(rcounts or [0] * nranks))
    mode = (2 if flat_ag else 0) | (4 if flat_rs else 0) | (8 if flat_ag == 2 else 0)
    args = (a, nranks, rank, count, rc, 0, esz, int(in_place), chunk_bytes, mode, slot, merge, _dtype(dtype),
            OPS[op])
    n = lib().bine_plan_dm_trees(*args, None, None, 0)
    if n < 0:
        raise BineError(int(-n), f"dm_tree_plan {coll}_{algo}")
    host, defer = (ctypes.c_int32 * max(int(n), 1))(), (ctypes.c_int32 * max(int(n), 1))()
    lib().bine_plan_dm_trees(*args, host, defer, n)
    return list(host[:n]), list(defer[:n])


def dm_fused_plan(coll: str, algo, nranks: int, rank: int, count: int = 0, rcounts=None, esz: int = 4,
                  in_place: bool = False, chunk_bytes: int = 0, flat_ag=False, flat_rs: bool = False,
                  slot: int = 64 << 20, dtype="float", op: str = "sum", small: bool = False) -> int:
    """k_dm_fused launches the direct transport issues for rank `rank`'s call
    (bine_plan_dm_fused, host only; fused trees on): 0 = the per-exchange
    launches instead."""
    a = _algo(coll, algo)
    rc = (ctypes.c_int * nranks)(*(rcounts or [0] * nranks))
    mode = (2 if flat_ag else 0) | (4 if flat_rs else 0) | (8 if flat_ag == 2 else 0)
    n = lib().bine_plan_dm_fused(a, nranks, rank, count, rc, 0, esz, int(in_place), chunk_bytes, mode, slot,
                                 _dtype(dtype), OPS[op], int(small))
    if n < 0:
        raise BineError(int(-n), f"dm_fused_plan {coll}_{algo}")
    return int(n)


def dm_fused_msgs(coll: str, algo, nranks: int, rank: int, count: int = 0, rcounts=None, esz: int = 4,
                  in_place: bool = False, chunk_bytes: int = 0, flat_ag=False, flat_rs: bool = False,
                  slot: int = 64 << 20, dtype="float", op: str = "sum", small: bool = False):
    """(launches, [(launch, push, peer, bytes), ...]) of the one-launch form
    (bine_plan_dm_fused_msgs): the messages in sequence-number order"""
    a = _algo(coll, algo)
    rc = (ctypes.c_int * nranks)(*(rcounts or [0] * nranks))
    mode = (2 if flat_ag else 0) | (4 if flat_rs else 0) | (8 if flat_ag == 2 else 0)
    args = (a, nranks, rank, count, rc, 0, esz, int(in_place), chunk_bytes, mode, slot, _dtype(dtype), OPS[op],
            int(small))
    n = ctypes.c_int64(0)
    nl = lib().bine_plan_dm_fused_msgs(*args, None, 0, ctypes.byref(n))
    if nl < 0:
        raise BineError(int(-nl), f"dm_fused_msgs {coll}_{algo}")
    buf = (ctypes.c_uint64 * max(4 * n.value, 4))()
    lib().bine_plan_dm_fused_msgs(*args, buf, n.value, ctypes.byref(n))
    return int(nl), [tuple(int(x) for x in buf[4 * k:4 * k + 4]) for k in range(n.value)]


def stage_plan(coll: str, algo, nranks: int, rank: int, count: int = 0, rcounts=None, esz: int = 4,
               segsize: int = 0, in_place: bool = False, chunk_bytes: int = 0, flat_ag=False, flat_rs: bool = False):
    """The host staging of rank `rank`'s schedule (bine_plan_stage; host only):
    (h2d, d2h, h2d_wait) with h2d / d2h = {op: [(lo, hi), ...]} element ranges
    copied before / after op, h2d_wait = [newest op whose h2d batch op i waits
    for, or -1]."""
    a = _algo(coll, algo)
    rc = (ctypes.c_int * nranks)(*(rcounts or [0] * nranks))
    mode = (2 if flat_ag else 0) | (4 if flat_rs else 0) | (8 if flat_ag == 2 else 0)
    res = []
    for kind, w in ((0, 3), (1, 3), (2, 2)):
        args = (a, nranks, rank, count, rc, 0, esz, segsize, int(in_place), chunk_bytes, mode, kind)
        n = lib().bine_plan_stage(*args, None, 0)
        if n < 0:
            raise BineError(int(-n), f"stage_plan {coll}_{algo}")
        arr = (ctypes.c_uint64 * max(int(n) * w, 1))()
        lib().bine_plan_stage(*args, arr, n)
        if kind < 2:
            d = {}
            for k in range(int(n)):
                d.setdefault(int(arr[3 * k]), []).append((int(arr[3 * k + 1]), int(arr[3 * k + 2])))
            res.append(d)
        else:
            res.append([ctypes.c_int64(arr[2 * k + 1]).value for k in range(int(n))])
    return tuple(res)


def reduce_batch(ins, inouts, counts, dtype, op: str = "sum", stream=None) -> int:
    """inouts[k][:counts[k]] = inouts[k] (op) ins[k], all windows in one launch.
    Returns the status (BINE_ERR_ARG = 1 when windows are not co-aligned)."""
    n = len(ins)
    c = (ctypes.c_size_t * n)(*counts)
    b = _ptrs(inouts)
    return lib().bine_reduce_batch(n, _ptrs(ins), b, b, c, _dtype(dtype, inouts[0]), OPS[op], _stream(stream, None))


def reduce_tree(leaves, out, count: int, dtype, op: str = "sum", stream=None, swap: int = 0, scale=None) -> int:
    """out[:count] = the reduction tree over the leaf buffers (tree order,
    len 2/4/8/16) in one launch (bine_reduce_tree; bit l of `swap`: level l
    takes its right operand as the inout side, bine_reduce_tree_swap; scale:
    the result times `scale` in the same launch, bine_reduce_tree_scaled).
    Returns the status."""
    if scale is not None:
        return lib().bine_reduce_tree_scaled(len(leaves), _ptrs(leaves), _ptr(out), count, _dtype(dtype, out),
                                             OPS[op], swap, float(scale), _stream(stream, None))
    if swap:
        return lib().bine_reduce_tree_swap(len(leaves), _ptrs(leaves), _ptr(out), count, _dtype(dtype, out),
                                           OPS[op], swap, _stream(stream, None))
    return lib().bine_reduce_tree(len(leaves), _ptrs(leaves), _ptr(out), count, _dtype(dtype, out), OPS[op],
                                  _stream(stream, None))


def exchange(comm: Comm, sends=(), recvs=(), stream=None) -> None:
    """One group of P2P transfers (bine_exchange): sends / recvs are
    (peer, buffer, nbytes) triples; receives match the peers' sends in size
    and posting order."""
    ns, nr = len(sends), len(recvs)
    sp = (ctypes.c_int * max(ns, 1))(*[p for p, _, _ in sends])
    sb = (ctypes.c_void_p * max(ns, 1))(*[_ptr(b) for _, b, _ in sends])
    sz = (ctypes.c_size_t * max(ns, 1))(*[n for _, _, n in sends])
    rp = (ctypes.c_int * max(nr, 1))(*[p for p, _, _ in recvs])
    rb = (ctypes.c_void_p * max(nr, 1))(*[_ptr(b) for _, b, _ in recvs])
    rz = (ctypes.c_size_t * max(nr, 1))(*[n for _, _, n in recvs])
    check(lib().bine_exchange(comm.handle, ns, sp, sb, sz, nr, rp, rb, rz, _stream(stream, comm)), "exchange")


def vendor_allreduce(sbuf, rbuf, count: int, dtype, op: str, comm: Comm, stream=None) -> None:
    """RCCL's own ncclAllReduce on the same communicator (bine_vendor_allreduce):
    a measurement baseline beside the Bine path, not a libbine algorithm."""
    check(lib().bine_vendor_allreduce(comm.handle, _ptr(sbuf), _ptr(rbuf), count, _dtype(dtype, rbuf), OPS[op],
                                      _stream(stream, comm)), "vendor_allreduce")


def allgather(algo, sbuf, rbuf, count: int, dtype, comm: Comm, stream=None) -> None:
    """count = elements per rank; rbuf holds comm.size * count elements."""
    check(lib().bine_allgather(comm.handle, _algo("allgather", algo), _ptr(sbuf), _ptr(rbuf), count,
                               _dtype(dtype, rbuf), _stream(stream, comm)), f"allgather_{algo}")


def loopback_allgather(comms, algo, sbufs, rbufs, count, dtype):
    st = (ctypes.c_int * len(comms))()
    hs = (ctypes.c_void_p * len(comms))(*[c.handle.value for c in comms])
    rc = lib().bine_loopback_run_allgather(hs, len(comms), _algo("allgather", algo), _ptrs(sbufs), _ptrs(rbufs),
                                           count, _dtype(dtype, rbufs[0]), st)
    return rc, list(st)


def bcast(algo, buf, count: int, dtype, root: int, comm: Comm, stream=None) -> None:
    """root's `count` elements of buf reach every rank (in place)."""
    check(lib().bine_bcast(comm.handle, _algo("bcast", algo), _ptr(buf), count, _dtype(dtype, buf), root,
                           _stream(stream, comm)), f"bcast_{algo}")


def loopback_bcast(comms, algo, bufs, count, dtype, root):
    st = (ctypes.c_int * len(comms))()
    hs = (ctypes.c_void_p * len(comms))(*[c.handle.value for c in comms])
    rc = lib().bine_loopback_run_bcast(hs, len(comms), _algo("bcast", algo), _ptrs(bufs), count,
                                       _dtype(dtype, bufs[0]), root, st)
    return rc, list(st)


def gather(algo, sbuf, rbuf, count: int, dtype, root: int, comm: Comm, stream=None) -> None:
    """every rank's `count` elements of sbuf land in block r of the root's rbuf
    (P * count elements; rbuf may be None elsewhere)."""
    check(lib().bine_gather(comm.handle, _algo("gather", algo), _ptr(sbuf), _ptr(rbuf), count,
                            _dtype(dtype, sbuf), root, _stream(stream, comm)), f"gather_{algo}")


def scatter(algo, sbuf, rbuf, count: int, dtype, root: int, comm: Comm, stream=None) -> None:
    """block r of the root's sbuf (P * count elements; sbuf may be None
    elsewhere) lands in rank r's rbuf (`count` elements)."""
    check(lib().bine_scatter(comm.handle, _algo("scatter", algo), _ptr(sbuf), _ptr(rbuf), count,
                             _dtype(dtype, rbuf), root, _stream(stream, comm)), f"scatter_{algo}")


def alltoall(algo, sbuf, rbuf, count: int, dtype, comm: Comm, stream=None) -> None:
    """block j of rank r's sbuf lands in block r of rank j's rbuf (both P * count
    elements)."""
    check(lib().bine_alltoall(comm.handle, _algo("alltoall", algo), _ptr(sbuf), _ptr(rbuf), count,
                              _dtype(dtype, rbuf), _stream(stream, comm)), f"alltoall_{algo}")


def _loopback(fn, coll, comms, algo, sbufs, rbufs, count, dtype, *root):
    st = (ctypes.c_int * len(comms))()
    hs = (ctypes.c_void_p * len(comms))(*[c.handle.value for c in comms])
    ref = next(b for b in list(rbufs) + list(sbufs) if b is not None)
    rc = fn(hs, len(comms), _algo(coll, algo), _ptrs(sbufs), _ptrs(rbufs), count, _dtype(dtype, ref), *root, st)
    return rc, list(st)


def loopback_gather(comms, algo, sbufs, rbufs, count, dtype, root):
    return _loopback(lib().bine_loopback_run_gather, "gather", comms, algo, sbufs, rbufs, count, dtype, root)


def loopback_scatter(comms, algo, sbufs, rbufs, count, dtype, root):
    return _loopback(lib().bine_loopback_run_scatter, "scatter", comms, algo, sbufs, rbufs, count, dtype, root)


def loopback_alltoall(comms, algo, sbufs, rbufs, count, dtype):
    return _loopback(lib().bine_loopback_run_alltoall, "alltoall", comms, algo, sbufs, rbufs, count, dtype)


# ---- libbine-named entry points (include/libbine.h:30-78) --------------------------

def _mk_ar(name):
    def f(sbuf, rbuf, count, dtype, op, comm, stream=None, segsize: int = 0, scale=None):
        allreduce(name, sbuf, rbuf, count, dtype, op, comm, segsize=segsize, stream=stream, scale=scale)
    f.__name__ = "allreduce_" + name
    f.__doc__ = f"allreduce_{name} (libbine_allreduce.c) on MI355X."
    return f


def _mk_rs(name):
    def f(sbuf, rbuf, rcounts, dtype, op, comm, stream=None, scale=None):
        reduce_scatter(name, sbuf, rbuf, rcounts, dtype, op, comm, stream=stream, scale=scale)
    f.__name__ = "reduce_scatter_" + name
    f.__doc__ = f"reduce_scatter_{name} (libbine_reduce_scatter.c) on MI355X."
    return f


def _mk_rd(name):
    def f(sbuf, rbuf, count, dtype, op, root, comm, stream=None):
        reduce(name, sbuf, rbuf, count, dtype, op, root, comm, stream=stream)
    f.__name__ = "reduce_" + name
    f.__doc__ = f"reduce_{name} (libbine_reduce.c) on MI355X."
    return f


def _mk_ag(name):
    def f(sbuf, rbuf, count, dtype, comm, stream=None):
        allgather(name, sbuf, rbuf, count, dtype, comm, stream=stream)
    f.__name__ = "allgather_" + name
    f.__doc__ = f"allgather_{name} (libbine_allgather.c) on MI355X."
    return f


def _mk_bc(name):
    def f(buf, count, dtype, root, comm, stream=None):
        bcast(name, buf, count, dtype, root, comm, stream=stream)
    f.__name__ = "bcast_" + name
    f.__doc__ = f"bcast_{name} (libbine_bcast.c) on MI355X."
    return f


ENTRY_POINTS = {}
for _n in ALGOS["allreduce"]:
    ENTRY_POINTS["allreduce_" + _n] = _mk_ar(_n)
for _n in ALGOS["reduce_scatter"]:
    ENTRY_POINTS["reduce_scatter_" + _n] = _mk_rs(_n)
for _n in ALGOS["reduce"]:
    ENTRY_POINTS["reduce_" + _n] = _mk_rd(_n)
for _n in ALGOS["allgather"]:
    ENTRY_POINTS["allgather_" + _n] = _mk_ag(_n)
for _n in ALGOS["bcast"]:
    ENTRY_POINTS["bcast_" + _n] = _mk_bc(_n)
ENTRY_POINTS["alltoall_bine"] = lambda sbuf, rbuf, count, dtype, comm, stream=None: \
    alltoall("bine", sbuf, rbuf, count, dtype, comm, stream=stream)
ENTRY_POINTS["gather_bine"] = lambda sbuf, rbuf, count, dtype, root, comm, stream=None: \
    gather("bine", sbuf, rbuf, count, dtype, root, comm, stream=stream)
ENTRY_POINTS["scatter_bine"] = lambda sbuf, rbuf, count, dtype, root, comm, stream=None: \
    scatter("bine", sbuf, rbuf, count, dtype, root, comm, stream=stream)
globals().update(ENTRY_POINTS)

__all__ = ["Comm", "BineError", "IN_PLACE", "schedule", "dm_fused_plan", "dm_fused_msgs", "reduce_local", "reduce3", "fill_pico", "checksum", "copy",
           "rccl_version", "scale", "scale_valid", "wide_valid", "widen", "narrow", "reduce_tree_wide",
           "allreduce_wide", "reduce_scatter_wide", "loopback_allreduce_wide", "loopback_reduce_scatter_wide",
           "wide_plan", "copy_segments", "plan_segments", "allreduce_multi", "loopback_allreduce_multi",
           "copy_shards", "plan_shards", "reduce_scatter_multi", "allgather_multi",
           "loopback_reduce_scatter_multi", "loopback_allgather_multi",
           "sumsq_segments", "plan_sumsq", "clip_segments", "norm_multi", "clip_multi", "loopback_norm_multi",
           "loopback_clip_multi",
           "adamw_consts", "plan_adamw", "adamw_segments", "adamw_multi", "loopback_adamw_multi",
           "step_state_init", "step_update_host", "step_update", "step_state_read", "adamw_segments_dyn",
           "adamw_multi_dyn", "loopback_adamw_multi_dyn",
           "amax_segments", "fp8_scales", "fp8_scale_host", "quant_segments", "dequant_segments", "plan_quant",
           "quant_multi", "loopback_quant_multi",
           "mx_dbytes", "mx_scale_host", "plan_mx", "mx_quant_segments", "mx_dequant_segments", "mx_quant_multi",
           "loopback_mx_quant_multi", "mx_wire_bytes", "plan_mx_sum", "mx_sum_segments", "mx_reduce_scatter_multi",
           "loopback_mx_reduce_scatter_multi",
           "mx_quant_ef_segments", "plan_mx_ef", "mx_reduce_scatter_multi_ef", "loopback_mx_reduce_scatter_multi_ef",
           "set_reduce_tuning", "allreduce", "reduce_scatter", "reduce", "loopback_allreduce",
           "loopback_reduce_scatter", "loopback_reduce", "plan", "allgather", "loopback_allgather", "bcast", "loopback_bcast", "reduce_batch",
           "gather", "scatter", "alltoall", "loopback_gather", "loopback_scatter", "loopback_alltoall",
           "exchange", "vendor_allreduce", "reduce_tree", "allreduce_staged", "reduce_scatter_staged",
           "stage_plan", "dm_tree_plan"] + list(ENTRY_POINTS)

"""The kernels' dispatch matrix: which (dtype, op, nl) every entry point of
pico_amd/csrc/kernels.hip accepts, what it returns for the rest, and that each
accepted combination reaches the kernel instantiated for it.

Every dtype id of include/bine_amd.h (10 basic, 5 pair, 2 complex, float16,
bfloat16) and one id outside every range, every op and one op id past the
last, through bine_reduce3, bine_reduce_batch, bine_reduce_tree (2 and 16
leaves), bine_scale, bine_reduce_tree_scaled and the occupancy query
bine_dm_launch_cap.  The expected statuses are written out below, not asked
of the library.  Values are compared bit for bit with the host arithmetic the
other GPU tests use (the oracle's MPI_Reduce_local, tests/h16_util.py,
tests/scale_sim.py).

Shape: 67 elements, every operand starting one element past a 16-B boundary,
so that for every element size from 1 to 16 bytes the scalar head, the 16-B
vector body and the scalar tail all run (16-byte elements have no head)."""
import ctypes

import numpy as np
import pytest

import h16_util as H
import scale_sim as SS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
from pico_amd._lib import DTYPES, EXT_DTYPES, OPS  # noqa: E402
from test_gpu import _host_tree, sha  # noqa: E402

N = 67
OK, ERR_ARG = 0, 1
BAD_DTYPE, BAD_OP = 40, 12            # past BINE_EXT_DTYPE_END, = BINE_NUM_OPS
CODES = {**DTYPES, **EXT_DTYPES}
OP_NAMES = sorted(OPS, key=OPS.get)   # by op id: sum prod max min land band lor bor lxor bxor maxloc minloc

# The status of bine_reduce3 / bine_reduce_batch / bine_reduce_tree per dtype,
# one character per op id 0..11 and then BAD_OP: '.' BINE_SUCCESS, 'A'
# BINE_ERR_ARG (every pair MPICH's MPI_Reduce_local refuses is BINE_ERR_ARG at
# all three entry points, from whichever compilation of the kernels the call
# is routed to; so are the ids outside the enums).
#             s p M m L b L b L b X N ?
_INT = "..........AAA"
_FLT = ".....A.A.AAAA"
_LOC = "AAAAAAAAAA..A"
_CPX = "..AAAAAAAAAAA"
_H16 = "....AAAAAAAAA"
STATUS = {"int8": _INT, "uint8": _INT, "int16": _INT, "uint16": _INT, "int32": _INT, "uint32": _INT,
          "int64": _INT, "uint64": _INT, "float": _FLT, "double": _FLT,
          "float_int": _LOC, "double_int": _LOC, "long_int": _LOC, "2int": _LOC, "short_int": _LOC,
          "c_float_complex": _CPX, "c_double_complex": _CPX, "float16": _H16, "bfloat16": _H16,
          "out_of_range": "AAAAAAAAAAAAA"}
assert set(STATUS) == set(CODES) | {"out_of_range"} and len(CODES) == 19

SCALE_TYPES = ("float", "double", "float16", "bfloat16")
DM_TYPES = ("float", "double", "int32", "int64", "uint32", "uint64")
ARITH = ("sum", "prod", "max", "min")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def code_of(dtype):
    return BAD_DTYPE if dtype == "out_of_range" else CODES[dtype]


def np_of(dtype):
    return np.dtype(np.uint16 if dtype in H.TYPES else O.NP_DTYPES[dtype])


def leaves_of(dtype, op, nl=16):
    """nl host operands of N elements: the 16-bit types' per-op inputs of
    tests/h16_util.py, else pico_core's generator sparsified (zeros, -0.0, NaN)"""
    if dtype in H.TYPES:
        return H.inputs(dtype, N, nl, op, seed=500)
    return [O.sparsify(O.fill(dtype, N, 500 + j), dtype, j) for j in range(nl)]


def pairwise(a, b, dtype, op):
    """b (op) a, b the inout side"""
    exp = b.copy()
    (H.reduce_local if dtype in H.TYPES else O.reduce_local)(a, exp, dtype, op)
    return exp


def tree(leaves, dtype, op):
    return H.tree(leaves, dtype, op) if dtype in H.TYPES else _host_tree(leaves, dtype, op)


def same(got, exp, dtype):
    return H.same(got, exp, dtype) if dtype in H.TYPES else sha(got) == sha(exp)


class Slots:
    """a device byte buffer of `k` slots, each holding N elements of `esz`
    bytes from one element past a 16-B boundary on"""

    def __init__(self, k, esz):
        self.esz = esz
        self.stride = (((N + 1) * esz + 15) // 16 + 1) * 16
        self.t = torch.zeros(k * self.stride, dtype=torch.uint8, device="cuda:0")
        assert self.t.data_ptr() % 16 == 0

    def off(self, i):
        return i * self.stride + self.esz

    def ptr(self, i):
        return self.t.data_ptr() + self.off(i)

    def put(self, arrays):
        host = np.zeros(len(arrays) * self.stride, np.uint8)
        for i, a in enumerate(arrays):
            raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            host[self.off(i):self.off(i) + raw.size] = raw
        self.t[:host.size] = torch.from_numpy(host).to("cuda:0")

    def get(self, first, k, nd):
        """slots first .. first + k - 1 as arrays of nd, and the bytes around them"""
        raw = self.t[first * self.stride:(first + k) * self.stride].cpu().numpy()
        out = []
        for i in range(k):
            o = i * self.stride + self.esz
            out.append(raw[o:o + N * self.esz].view(nd).copy())
            raw[o:o + N * self.esz] = 0
        return out, raw


def vp(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def stream():
    return torch.cuda.current_stream().cuda_stream


NOUT = 5   # reduce3, batch window 0, batch window 1, tree of 2, tree of 16


def run_reduce_family(L, s, code, opv):
    """the four launches on slots 0..15 (operands) -> 16..20 (results); their statuses"""
    st = stream()
    cnt = (ctypes.c_size_t * 2)(N, N)
    return [L.bine_reduce3(s.ptr(0), s.ptr(1), s.ptr(16), N, code, opv, st),
            L.bine_reduce_batch(2, vp([s.ptr(0), s.ptr(2)]), vp([s.ptr(1), s.ptr(3)]), vp([s.ptr(17), s.ptr(18)]),
                                cnt, code, opv, st),
            L.bine_reduce_tree(2, vp([s.ptr(j) for j in range(2)]), s.ptr(19), N, code, opv, st),
            L.bine_reduce_tree(16, vp([s.ptr(j) for j in range(16)]), s.ptr(20), N, code, opv, st)]


@pytest.mark.parametrize("dtype", list(STATUS))
def test_reduce_family_statuses_and_values(dev, dtype):
    """bine_reduce3, bine_reduce_batch (n = 2), bine_reduce_tree (nl = 2, 16):
    BINE_SUCCESS exactly where bine_op_valid is 1 and the table says so, the
    table's error elsewhere, and the host's bits wherever the call succeeds"""
    L = pico_amd.lib()
    code = code_of(dtype)
    esz = np_of(dtype).itemsize if dtype != "out_of_range" else 16
    s = Slots(16 + NOUT, esz)
    for opv, ch in enumerate(STATUS[dtype]):
        want = OK if ch == "." else ERR_ARG
        assert bool(L.bine_op_valid(code, opv)) == (want == OK), (dtype, opv)
        if want != OK:
            assert run_reduce_family(L, s, code, opv) == [want] * 4, (dtype, opv)
            continue
        op = OP_NAMES[opv]
        h = leaves_of(dtype, op)
        s.put(h + [np.zeros(N, np_of(dtype))] * NOUT)
        assert run_reduce_family(L, s, code, opv) == [OK] * 4, (dtype, op)
        torch.cuda.synchronize()
        got, around = s.get(16, NOUT, np_of(dtype))
        exp = [pairwise(h[0], h[1], dtype, op), pairwise(h[0], h[1], dtype, op), pairwise(h[2], h[3], dtype, op),
               tree(h[:2], dtype, op), tree(h, dtype, op)]
        for k, what in enumerate(("reduce3", "batch[0]", "batch[1]", "tree 2", "tree 16")):
            assert same(got[k], exp[k], dtype), (dtype, op, what)
        assert not around.any(), (dtype, op, "bytes outside the results")


def test_reduce_tree_leaf_counts(dev):
    """2, 4, 8 and 16 leaves (float SUM) give the host's tree; 1, 3 and 32
    leaves are BINE_ERR_ARG"""
    L = pico_amd.lib()
    code, opv = CODES["float"], OPS["sum"]
    h = leaves_of("float", "sum", 32)
    s = Slots(33, 4)
    s.put(h + [np.zeros(N, np.float32)])
    for nl in (2, 4, 8, 16):
        assert L.bine_reduce_tree(nl, vp([s.ptr(j) for j in range(nl)]), s.ptr(32), N, code, opv, stream()) == OK
        torch.cuda.synchronize()
        got, around = s.get(32, 1, np.float32)
        assert same(got[0], tree(h[:nl], "float", "sum"), "float") and not around.any(), nl
    for nl in (1, 3, 32):
        assert L.bine_reduce_tree(nl, vp([s.ptr(j) for j in range(nl)]), s.ptr(32), N, code, opv,
                                  stream()) == ERR_ARG, nl


@pytest.mark.parametrize("dtype", list(STATUS))
def test_scale_and_scaled_tree(dev, dtype):
    """bine_scale and bine_reduce_tree_scaled succeed exactly on {float,
    double, float16, bfloat16} (x {sum, prod, max, min}) with the bits of
    tests/scale_sim.py's S, and are BINE_ERR_ARG everywhere else"""
    L = pico_amd.lib()
    code, scale = code_of(dtype), 1 / 3
    ok_t = dtype in SCALE_TYPES
    nd = np_of(dtype) if dtype != "out_of_range" else np.dtype(np.uint8)
    s = Slots(4, nd.itemsize if dtype != "out_of_range" else 16)
    assert L.bine_scale(s.ptr(0), s.ptr(2), N, code, scale, stream()) == (OK if ok_t else ERR_ARG)
    for opv in range(BAD_OP + 1):
        valid = ok_t and opv < 4
        assert bool(L.bine_scale_valid(code, opv)) == valid, (dtype, opv)
        if not valid:
            assert L.bine_reduce_tree_scaled(2, vp([s.ptr(0), s.ptr(1)]), s.ptr(3), N, code, opv, 0, scale,
                                             stream()) == ERR_ARG, (dtype, opv)
            continue
        op = OP_NAMES[opv]
        h = H.inputs(dtype, N, 2, op, seed=700) if dtype in H.TYPES else \
            [(np.random.default_rng(700 + j).random(N) * 100.0 - 30.0).astype(nd) for j in range(2)]
        s.put(h + [np.zeros(N, nd)] * 2)
        assert L.bine_scale(s.ptr(0), s.ptr(2), N, code, scale, stream()) == OK
        assert L.bine_reduce_tree_scaled(2, vp([s.ptr(0), s.ptr(1)]), s.ptr(3), N, code, opv, 0, scale,
                                         stream()) == OK
        torch.cuda.synchronize()
        got, around = s.get(2, 2, nd)
        assert got[0].tobytes() == SS.S(h[0], dtype, scale).tobytes(), (dtype, "bine_scale")
        assert got[1].tobytes() == SS.S(tree(h, dtype, op), dtype, scale).tobytes(), (dtype, op, "scaled tree")
        assert not around.any(), (dtype, op)


def test_dm_launch_cap_matrix(dev):
    """bine_dm_launch_cap (an occupancy query, nothing is launched): kind 0
    (k_dm_move) always has a cap; kind 1 (k_dm_move_tree) exactly for the six
    direct-transport types x the four arithmetic ops x nl in {2, 4, 8, 16};
    kind 2 (k_dm_fused) for those types and ops whatever nl; -1 elsewhere"""
    L = pico_amd.lib()
    bad = []
    for dtype in STATUS:
        for opv in range(-1, BAD_OP + 1):
            for nl in (2, 4, 8, 16, 3):
                pair = dtype in DM_TYPES and 0 <= opv < len(ARITH)
                for kind, want in ((0, True), (1, pair and nl != 3), (2, pair)):
                    cap = L.bine_dm_launch_cap(kind, code_of(dtype), opv, nl, 1)
                    if (cap > 0) != want or (not want and cap != -1):
                        bad.append((kind, dtype, opv, nl, cap))
    assert not bad, bad[:8]

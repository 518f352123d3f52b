"""k_reduce's tuning variants, its capped grid and the non-temporal k_sumsq_segs
on the GPU, bit for bit against host arithmetic the suite already trusts (the
oracle's MPI_Reduce_local, tests/h16_util.py, exact integer sums).

  * float SUM under every (U, NT) bine_set_reduce_tuning selects, with the
    default cap, one workgroup and three, at the counts and phases of
    tests/reduce_variants_cases.py (what they reach is proved on the CPU by
    tests/test_reduce_variants_cases.py: second trips of the grid-stride loop,
    a partial tile after full trips, a workgroup split across the loop
    boundary, the edges around one tile), bine_reduce3 out of place and
    bine_reduce_local in place;
  * every (type, op) of the compilation the setter reaches -- SUM, PROD, MAX,
    MIN on the ten basic types -- through the multi-trip shape under a cap of
    two workgroups;
  * operands that are not co-aligned, where the knobs must change nothing;
  * the other two compilations of the kernels (float16 / bfloat16; the
    logical, bitwise and MAXLOC / MINLOC ops, the pair and the complex types),
    whose cap comes from BINE_REDUCE_MAXBLOCKS alone, in a fresh process
    (tools/reduce_env_check.py);
  * bine_sumsq_segments and bine_norm_multi with BINE_SUMSQ_NT unset, 0 and 1.

Operands and output live in one arena of guard bytes (64 or more on either
side of each); after every launch the whole arena is compared with the host's
image, so a, the out-of-place b and every guard byte must be as they were.

These tests compare values.  They cannot observe which instantiation of
k_reduce ran or how many workgroups a launch had: a setter or an environment
variable that was silently ignored would pass them (every variant computes
the same bits).  What they do show is that each selectable variant, and the
capped grid, computes the right bits and writes nowhere else."""
import contextlib
import os
import sys
import time

import numpy as np
import pytest

import _sub
import reduce_variants_cases as C
from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
import test_gpu as TG  # noqa: E402  (the communicator cache)
import test_gpu_norm as TN  # noqa: E402  (the norm tests' buckets)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASIC = ["int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float", "double"]
ARITH = ("sum", "prod", "max", "min")
# tools/reduce_env_check.py took 2.3 s on the MI355X (profiles/reduce_variants.txt): three times
# that, floored at 60 s
ENV_CHECK_LIMIT = 60


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def default_tuning():
    yield
    pico_amd.set_reduce_tuning(4, 0, 1)


def reduced(a, b, dtype, op):
    """b (op) a by the oracle, b the inout side"""
    exp = b.copy()
    O.reduce_local(a, exp, dtype, op)
    return exp


_FLOAT_SUM = {}


def float_sum_case(U, nvec, phase):
    """the arena of (U, nvec, phase) and the device images a call must leave, made once and
    shared by every (NT, cap) that runs the shape"""
    key = (U, nvec, phase)
    if key not in _FLOAT_SUM:
        n = C.elements(nvec, 4, phase)
        a, b = O.fill("float", n, 11 + nvec), O.fill("float", n, 97 + nvec)
        ar = C.Arena(a, b, (phase,) * 3)
        ar.upload()
        exp = reduced(a, b, "float", "sum")
        host = {ip: ar.expected(exp, ip) for ip in (False, True)}
        _FLOAT_SUM[key] = (ar, n, host, {ip: ar.upload(img) for ip, img in host.items()})
    return _FLOAT_SUM[key]


def launch(ar, n, dtype, op, inplace):
    ar.reset()
    if inplace:
        pico_amd.reduce_local(ar.ptr(0), ar.ptr(1), n, dtype, op)
    else:
        pico_amd.reduce3(ar.ptr(0), ar.ptr(1), ar.ptr(2), n, dtype, op)


@pytest.mark.parametrize("NT", C.NTS)
@pytest.mark.parametrize("U", C.US)
def test_float_sum_every_variant(dev, U, NT):
    launches = 0
    for cap in C.CAPS:
        pico_amd.set_reduce_tuning(U, cap, NT)
        for nvec in C.counts(U):
            for phase in C.PHASES:
                ar, n, host, want = float_sum_case(U, nvec, phase)
                for inplace in (False, True):
                    launch(ar, n, "float", "sum", inplace)
                    launches += 1
                    if not ar.matches(want[inplace]):
                        pytest.fail(f"U={U} NT={NT} cap={cap} nvec={nvec} phase={phase} inplace={inplace}: "
                                    f"{ar.first_difference(host[inplace])}")
    assert launches == len(C.CAPS) * len(C.counts(U)) * 4


def basic_inputs(dtype, n):
    return O.sparsify(O.fill(dtype, n, 311), dtype, 0), O.sparsify(O.fill(dtype, n, 733), dtype, 1)


@pytest.mark.parametrize("dtype", BASIC)
def test_capped_grid_every_basic_type_and_op(dev, dtype):
    """the multi-trip shapes of the default U under a cap of two workgroups, one element past a
    16-B boundary: 16, 8, 4 and 2 elements per vector through the second trip, the partial tile
    and the split workgroup (the complex types' 16-byte elements belong to another compilation,
    which the setter does not reach: tools/reduce_env_check.py)"""
    L = pico_amd.lib()
    esz = np.dtype(O.NP_DTYPES[dtype]).itemsize
    pico_amd.set_reduce_tuning(C.DEFAULT_U, 2, 1)
    # the shape that reaches (b) .. (e), and the one whose last vector the guarded loop writes
    for nvec in (C.multi(C.DEFAULT_U), C.partial(C.DEFAULT_U)):
        n = C.elements(nvec, esz, 1)
        assert C.split(esz, n, esz) == (16 // esz - 1, nvec) and C.blocks_of(nvec, C.DEFAULT_U, 2) == 2
        a, b = basic_inputs(dtype, n)
        ar = C.Arena(a, b, (1, 1, 1))
        ar.upload()
        for op in ARITH:
            assert L.bine_op_valid(pico_amd.DTYPES[dtype], pico_amd.OPS[op]) == 1
            exp = reduced(a, b, dtype, op)
            for inplace in (False, True):
                launch(ar, n, dtype, op, inplace)
                diff = ar.first_difference(ar.expected(exp, inplace))
                assert diff is None, (dtype, op, nvec, inplace, diff)


@pytest.mark.parametrize("U", C.US)
def test_not_co_aligned_operands_ignore_the_knobs(dev, U):
    """operands at different offsets mod 16 B: one workgroup's scalar loop up to 4096 elements,
    k_reduce_scalar above -- with U, a cap of three workgroups and non-temporal stores set"""
    pico_amd.set_reduce_tuning(U, 3, 7)
    for n in (C.SCALAR_ABOVE, C.SCALAR_ABOVE + 1, 5003):
        a, b = O.fill("float", n, 5 + n), O.fill("float", n, 6 + n)
        exp = reduced(a, b, "float", "sum")
        for phases in ((1, 0, 0), (0, 3, 0), (2, 1, 3)):
            ar = C.Arena(a, b, phases)
            ar.upload()
            for inplace in (False, True):
                launch(ar, n, "float", "sum", inplace)
                diff = ar.first_difference(ar.expected(exp, inplace))
                assert diff is None, (U, n, phases, inplace, diff)


@pytest.mark.timeout(ENV_CHECK_LIMIT + 20)
def test_other_compilations_capped_by_the_environment(dev):
    """float16 / bfloat16 and the logical / bitwise / loc ops, pair and complex types take their
    cap from BINE_REDUCE_MAXBLOCKS at their first call: a fresh process with a cap of two
    workgroups (and U = 8 for float SUM) runs the multi-trip shapes of all of them"""
    env = dict(os.environ, PYTHONPATH=ROOT, BINE_REDUCE_MAXBLOCKS="2", BINE_REDUCE_UNROLL="8")
    env.pop("BINE_REDUCE_NT", None)
    t0 = time.time()
    r = _sub.run_kw([sys.executable, "-u", os.path.join(ROOT, "tools", "reduce_env_check.py")], env=env,
                    capture_output=True, text=True, timeout=ENV_CHECK_LIMIT, ranks=1)
    print(f"tools/reduce_env_check.py: {time.time() - t0:.1f} s")
    lines = [x for x in r.stdout.splitlines() if "MISMATCH" in x or "RESULT" in x]
    print("\n".join(lines[-5:]))
    assert r.returncode == 0, "\n".join(lines[:40]) + "\n" + r.stderr[-2000:]
    assert any(x.startswith("RESULT ") and " bad=0 " in x for x in lines), lines[-3:]


# ---- BINE_SUMSQ_NT ---------------------------------------------------------------------------------

@contextlib.contextmanager
def sumsq_nt(value):
    """BINE_SUMSQ_NT = value (None: unset) for the calls inside: the library reads it at every call"""
    saved = os.environ.get("BINE_SUMSQ_NT")
    try:
        if value is None:
            os.environ.pop("BINE_SUMSQ_NT", None)
        else:
            os.environ["BINE_SUMSQ_NT"] = value
        yield
    finally:
        if saved is None:
            os.environ.pop("BINE_SUMSQ_NT", None)
        else:
            os.environ["BINE_SUMSQ_NT"] = saved


def sumsq_under(b, value):
    with sumsq_nt(value):
        return TN.run_sumsq(b)


@pytest.mark.parametrize("dtype", TN.TYPES)
def test_sumsq_nontemporal_exact_on_small_integers(dev, dtype):
    """integers in [-8, 8]: every order of addition gives the host's bits, so unset, 0 and 1 must
    all give exactly them"""
    for specs in (TN.mixed_specs(dtype, 1), TN.many_specs(dtype, 2)):
        b = TN.bucket(dtype, specs, 3, "int")
        want = [float(np.sum(b.values(k) ** 2)) for k in range(len(specs))]
        want.append(float(sum(want)))
        want = np.array(want, dtype=np.float64).tobytes()
        for value in (None, "0", "1"):
            got = sumsq_under(b, value)
            assert got.tobytes() == want, (dtype, value, len(specs))
            assert b.unchanged(), (dtype, value, "sumsq wrote to its input or around it")


@pytest.mark.parametrize("dtype", TN.TYPES)
def test_sumsq_nontemporal_same_bits_on_normal_data(dev, dtype):
    """the bits depend on the data, the counts, the type and the addresses mod 16 B alone: not on
    the loads' cache policy"""
    b = TN.bucket(dtype, TN.mixed_specs(dtype, 4), 5, "normal")
    plain = sumsq_under(b, None)
    assert np.isfinite(plain.view(np.float64)).all() and plain.view(np.float64)[-1] > 0
    assert sumsq_under(b, "1").tobytes() == plain.tobytes(), dtype
    assert sumsq_under(b, "0").tobytes() == plain.tobytes(), dtype
    assert b.unchanged()


def test_norm_multi_nontemporal(dev):
    P, dtype = 2, "float"
    cs = TG.comms(P)
    bs = TN.rank_buckets(dtype, P, 60)
    n = len(bs[0].counts)
    got = {}
    for value in (None, "1"):
        stats = [TN.Guarded(n + 1) for _ in range(P)]
        with sumsq_nt(value):
            _, st = pico_amd.loopback_norm_multi(cs, "bine_lat", [b.ptrs() for b in bs], dtype,
                                                 [s.ptr() for s in stats], counts=[b.counts for b in bs])
            torch.cuda.synchronize()
        assert st == [0] * P, (value, st)
        got[value] = [s.read().tobytes() for s in stats]
        assert all(b.unchanged() for b in bs)
    assert got["1"] == got[None] and got[None][0] == got[None][1]
    assert np.frombuffer(got[None][0], dtype=np.float64)[-1] > 0

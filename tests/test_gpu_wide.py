"""Wide (binary32-accumulating) reductions on the GPU: k_widen / k_narrow, the
wide tree and the wide collectives over loopback ranks on one GPU, bit for bit
against the host statement of the definition (tests/wide_sim.py: widen, the
float replay, one narrowing) wherever the expected value is not NaN, NaN
wherever it is -- and path B against path A (BINE_WIDE_TREES=0)."""
import os

import numpy as np
import pytest

import h16_util as H
import wide_sim as WS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pico_amd  # noqa: E402
import test_gpu as TG  # noqa: E402  (the communicator cache)
from pico_amd._lib import BineError  # noqa: E402

OPS4 = ["sum", "prod", "max", "min"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def shifted(arr, shift, pad=512, fill=0):
    """a device byte buffer holding `arr` from element `shift` on; (tensor, address of the first element)"""
    e = arr.dtype.itemsize
    t = torch.full(((arr.size + shift) * e + pad,), fill, dtype=torch.uint8, device="cuda:0")
    if arr.size:
        t[shift * e:(shift + arr.size) * e] = torch.from_numpy(arr.view(np.uint8).copy()).to("cuda:0")
    return t, t.data_ptr() + shift * e


def read(t, nd, n, shift=0):
    e = np.dtype(nd).itemsize
    return t[shift * e:(shift + n) * e].cpu().numpy().view(nd).copy()


def same_f32(got, exp):
    nan = np.isnan(exp)
    return bool(np.array_equal(got[~nan].view(np.uint32), exp[~nan].view(np.uint32)) and np.isnan(got[nan]).all())


# ---- k_widen / k_narrow -----------------------------------------------------------------

@pytest.mark.parametrize("dtype", H.TYPES)
def test_widen_every_pattern(dev, dtype):
    """all 65,536 bit patterns: exact, NaN stays NaN; at 0 and 1 element past a 16-B boundary"""
    x = np.arange(1 << 16, dtype=np.uint16)
    exp = H.to_f32(x, dtype)
    for sh in (0, 1):
        ti, pi = shifted(x, sh)
        to, po = shifted(np.zeros(x.size, np.float32), sh, fill=0xA5)
        pico_amd.widen(pi, po, x.size, dtype)
        torch.cuda.synchronize()
        assert same_f32(read(to, np.float32, x.size, sh), exp), (dtype, sh)
        assert (to[(sh + x.size) * 4:].cpu().numpy() == 0xA5).all()
    ti, pi = shifted(x, 1)   # boundaries that do not coincide: the scalar kernel
    to, po = shifted(np.zeros(x.size, np.float32), 0)
    pico_amd.widen(pi, po, x.size, dtype)
    torch.cuda.synchronize()
    assert same_f32(read(to, np.float32, x.size), exp)


def narrow_grid(dtype):
    """binary32 values around every kind of rounding: exact ties between two
    16-bit neighbours (both parities), one binary32 ulp above and below them,
    the subnormal range of the 16-bit format, the overflow threshold, +-0,
    +-inf, NaN"""
    rng = np.random.default_rng(5)
    b = H.random_bits(dtype, 4096, 77)
    lo = H.to_f32(b, dtype)
    hi = H.to_f32((b + 1).astype(np.uint16), dtype)
    ok = np.isfinite(lo) & np.isfinite(hi)
    mid = ((lo[ok].astype(np.float64) + hi[ok].astype(np.float64)) / 2).astype(np.float32)   # exact in binary32
    up = np.nextafter(mid, np.float32(np.inf)).astype(np.float32)
    dn = np.nextafter(mid, np.float32(-np.inf)).astype(np.float32)
    fmax = float(H.to_f32(np.array([0x7BFF if dtype == "float16" else 0x7F7F], np.uint16), dtype)[0])
    ulp = fmax * (2.0 ** -10 if dtype == "float16" else 2.0 ** -7) / (2 - (2.0 ** -10 if dtype == "float16" else 2.0 ** -7))
    edge = np.array([fmax, fmax + ulp / 4, fmax + ulp / 2, np.nextafter(np.float32(fmax + ulp / 2), np.float32(0)),
                     -fmax - ulp / 2, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45], dtype=np.float32)
    tiny = float(H.to_f32(np.array([1], np.uint16), dtype)[0])   # the smallest 16-bit subnormal
    sub = (rng.random(2048) * 64 * tiny * rng.choice([-1.0, 1.0], 2048)).astype(np.float32)
    subt = (np.arange(64) * tiny / 2).astype(np.float32)        # exact ties in the subnormal range
    return np.concatenate([mid, up, dn, edge, sub, subt, -subt])


@pytest.mark.parametrize("dtype", H.TYPES)
def test_narrow(dev, dtype):
    rnd = np.random.default_rng(9).integers(0, 1 << 32, 1 << 20, dtype=np.uint32).view(np.float32)
    for x in (narrow_grid(dtype), rnd):
        exp = H.from_f32(x, dtype)
        for sh in (0, 1):
            ti, pi = shifted(x, sh)
            to, po = shifted(np.zeros(x.size, np.uint16), sh, fill=0xA5)
            pico_amd.narrow(pi, po, x.size, dtype)
            torch.cuda.synchronize()
            assert H.same(read(to, np.uint16, x.size, sh), exp, dtype), (dtype, sh, x.size)
            assert (to[(sh + x.size) * 2:].cpu().numpy() == 0xA5).all()
    x = rnd[:100003]
    ti, pi = shifted(x, 1)   # boundaries that do not coincide
    to, po = shifted(np.zeros(x.size, np.uint16), 0)
    pico_amd.narrow(pi, po, x.size, dtype)
    torch.cuda.synchronize()
    assert H.same(read(to, np.uint16, x.size), H.from_f32(x, dtype), dtype)


# ---- bine_reduce_tree_wide ------------------------------------------------------------------

TREE_COUNTS = [(67, 1)] + [(8 * v, 0) for v in (1, 3, 255, 256, 257, 1025)]


def tree_leaves(dtype, nl, n, op):
    """pico-like / near-one / random leaves with the special-value grid planted
    in leaves 0 and 1 (and, rotated, in the last two)"""
    lv = H.inputs(dtype, n, nl, op, seed=4321 + nl)
    a, b = H.special_grid(dtype)
    k = min(n, a.size)
    lv[0][:k], lv[1][:k] = a[:k], b[:k]
    if n >= 2 * a.size:
        lv[nl - 1][a.size:2 * a.size], lv[nl - 2][a.size:2 * a.size] = a, b
    return lv


@pytest.mark.parametrize("dtype", H.TYPES)
@pytest.mark.parametrize("nl", [2, 4, 8, 16])
def test_reduce_tree_wide(dev, dtype, nl):
    bad = []
    levels = nl.bit_length() - 1
    for n, sh in TREE_COUNTS:
        for op in OPS4:
            lv = tree_leaves(dtype, nl, n, op)
            dl = [shifted(x, sh) for x in lv]
            for swap in (0, (1 << levels) - 1):
                for scale in (1.0, 1 / 3, -0.1):
                    exp = WS.tree(lv, dtype, op, swap, scale)
                    to, po = shifted(np.zeros(n, np.uint16), sh, fill=0xA5)
                    rc = pico_amd.reduce_tree_wide([p for _, p in dl], po, n, dtype, op, swap=swap, scale=scale)
                    torch.cuda.synchronize()
                    if rc or not H.same(read(to, np.uint16, n, sh), exp, dtype):
                        bad.append((n, op, swap, scale, rc))
                    if not (to[(sh + n) * 2:(sh + n) * 2 + 256].cpu().numpy() == 0xA5).all():
                        bad.append((n, op, swap, scale, "guard"))
            # `out` aliasing a leaf (the last one), on a fresh copy
            ta, pa = shifted(lv[nl - 1], sh)
            ptrs = [p for _, p in dl[:-1]] + [pa]
            rc = pico_amd.reduce_tree_wide(ptrs, pa, n, dtype, op, swap=0, scale=1 / 3)
            torch.cuda.synchronize()
            if rc or not H.same(read(ta, np.uint16, n, sh), WS.tree(lv, dtype, op, 0, 1 / 3), dtype):
                bad.append((n, op, "alias", rc))
    assert not bad, bad[:8]


def test_reduce_tree_wide_not_coaligned(dev):
    """leaves at different phases of a 16-B line: the scalar kernel"""
    for dtype in H.TYPES:
        lv = tree_leaves(dtype, 4, 5000, "sum")
        dl = [shifted(x, j) for j, x in enumerate(lv)]
        to, po = shifted(np.zeros(5000, np.uint16), 0)
        assert pico_amd.reduce_tree_wide([p for _, p in dl], po, 5000, dtype, "sum", scale=0.25) == 0
        torch.cuda.synchronize()
        assert H.same(read(to, np.uint16, 5000), WS.tree(lv, dtype, "sum", 0, 0.25), dtype)


# ---- the collectives ----------------------------------------------------------------------------

N = 8195
CHUNK = 4096
CASES = [("allreduce", "bine_bdw_remap"), ("allreduce", "bine_lat"), ("allreduce", "ring"),
         ("reduce_scatter", "bine_permute_remap"), ("reduce_scatter", "bine_block_by_block")]


def rcounts_of(P):
    per = N // P
    rc = [per + (i % 3) for i in range(P)]
    rc[-1] += N - sum(rc)
    return rc


def to_dev(a, pad=64):
    raw = np.ascontiguousarray(a).view(np.uint8)
    t = torch.zeros(raw.size + pad, dtype=torch.uint8, device="cuda:0")
    if raw.size:
        t[:raw.size] = torch.from_numpy(raw.copy()).to("cuda:0")
    return t


def run(coll, algo, sb, dtype, op, rc, in_place, scale):
    P = len(sb)
    ds = [to_dev(x) for x in sb]
    nout = rc if coll == "reduce_scatter" else [sb[0].size] * P
    dr = ds if in_place else [torch.full((max(c, 1) * 2 + 64,), 0xA5, dtype=torch.uint8, device="cuda:0") for c in nout]
    torch.cuda.synchronize()
    src = [pico_amd.IN_PLACE] * P if in_place else ds
    if coll == "allreduce":
        _, st = pico_amd.loopback_allreduce_wide(TG.comms(P), algo, src, dr, sb[0].size, dtype, op, scale=scale)
    else:
        _, st = pico_amd.loopback_reduce_scatter_wide(TG.comms(P), algo, src, dr, rc, dtype, op, scale=scale)
    torch.cuda.synchronize()
    return [d[:c * 2].cpu().numpy().view(np.uint16).copy() for d, c in zip(dr, nout)], st


def set_form(cs, flat):
    for c in cs:
        c.set_flat_rs(flat)
        c.set_flat_ag(2 if flat else 0)
        c.set_chunk(CHUNK if flat else 0)


@pytest.mark.parametrize("dtype", H.TYPES)
@pytest.mark.parametrize("P", [1, 2, 3, 4, 6, 8])
def test_collectives(dev, P, dtype):
    """count 8195 (ragged rcounts), chunk 4096, flat and literal, in and out of
    place, scale 1.0 and 1/P: against the host statement, and path B against
    path A.  Where the float call's plan fails (a power-of-two algorithm at
    P = 3, 6) the wide call returns that status on every rank."""
    bad, paths = [], set()
    cs = TG.comms(P)
    saved = os.environ.get("BINE_WIDE_TREES")
    cache = {}
    try:
        for flat in (False, True):
            set_form(cs, flat)
            for coll, algo in CASES:
                rc = rcounts_of(P) if coll == "reduce_scatter" else None
                kw = dict(rcounts=rc) if rc else dict(count=N)
                for ip in (False, True):
                    key = (coll, algo, ip)
                    if key not in cache:   # one host replay serves both forms and both scales
                        sb = H.inputs(dtype, N, P, "sum")
                        try:
                            cache[key] = (sb, WS.collective(coll, algo, sb, dtype, "sum", rc, ip), 0)
                        except BineError as e:
                            cache[key] = (sb, None, e.status)
                    sb, f16, status = cache[key]
                    if status:
                        _, st = run(coll, algo, sb, dtype, "sum", rc, ip, 1.0)
                        if st != [status] * P:
                            bad.append((coll, algo, flat, ip, "status", st, status))
                        continue
                    path_b = pico_amd.wide_plan(coll, algo, P, flat_ag=2 if flat else 0, flat_rs=flat, **kw)
                    paths.add(path_b)
                    for s in (1.0, 1.0 / P):
                        exp = WS.collective(coll, algo, sb, dtype, "sum", rc, ip, s) if s != 1.0 else f16
                        os.environ.pop("BINE_WIDE_TREES", None)
                        outs, st = run(coll, algo, sb, dtype, "sum", rc, ip, s)
                        os.environ["BINE_WIDE_TREES"] = "0"
                        outa, sta = run(coll, algo, sb, dtype, "sum", rc, ip, s)
                        if any(st) or any(sta):
                            bad.append((coll, algo, flat, ip, s, "status", st, sta))
                            continue
                        if not all(H.same(outs[r], exp[r], dtype) for r in range(P)):
                            bad.append((coll, algo, flat, ip, s, "bits", "B" if path_b else "A"))
                        if not all(H.same(outa[r], exp[r], dtype) for r in range(P)):
                            bad.append((coll, algo, flat, ip, s, "bits of path A"))
    finally:
        set_form(cs, False)
        if saved is None:
            os.environ.pop("BINE_WIDE_TREES", None)
        else:
            os.environ["BINE_WIDE_TREES"] = saved
    assert not bad, bad[:8]
    if P in (2, 4, 8):
        assert paths == {False, True}, paths   # both paths ran


@pytest.mark.parametrize("P", [4])
def test_collectives_max_prod(dev, P):
    """MAX / MIN on random bit patterns and PROD near one, flat (path B) and
    literal, each again under BINE_WIDE_TREES=0 (path A)"""
    bad = []
    cs = TG.comms(P)
    saved = os.environ.get("BINE_WIDE_TREES")
    try:
        for flat in (False, True):
            set_form(cs, flat)
            for dtype in H.TYPES:
                for op in ("max", "prod", "min"):
                    sb = H.inputs(dtype, N, P, op)
                    exp = WS.collective("allreduce", "bine_bdw_remap", sb, dtype, op, scale=-0.1)
                    for forced_a in (False, True):
                        if forced_a:
                            os.environ["BINE_WIDE_TREES"] = "0"
                        else:
                            os.environ.pop("BINE_WIDE_TREES", None)
                        outs, st = run("allreduce", "bine_bdw_remap", sb, dtype, op, None, False, -0.1)
                        if any(st) or not all(H.same(outs[r], exp[r], dtype) for r in range(P)):
                            bad.append((flat, dtype, op, forced_a, st))
    finally:
        set_form(cs, False)
        if saved is None:
            os.environ.pop("BINE_WIDE_TREES", None)
        else:
            os.environ["BINE_WIDE_TREES"] = saved
    assert not bad, bad


def test_refusals(dev):
    """every invalid (dtype, op) pair: BINE_ERR_ARG on every rank, and every
    output buffer keeps its 0xA5 fill (what a launch would have overwritten)"""
    P, n = 4, 64
    cs = TG.comms(P)
    codes = {**pico_amd.DTYPES, **pico_amd.EXT_DTYPES}
    for dname in codes:
        for op in pico_amd.OPS:
            if pico_amd.wide_valid(dname, op):
                continue
            ds = [torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0") for _ in range(P)]
            dr = [torch.full((n * 16,), 0xA5, dtype=torch.uint8, device="cuda:0") for _ in range(P)]
            rc, st = pico_amd.loopback_allreduce_wide(cs, "bine_bdw_remap", ds, dr, n, dname, op)
            assert rc == 1 and st == [1] * P, (dname, op, rc, st)
            rc, st = pico_amd.loopback_reduce_scatter_wide(cs, "bine_permute_remap", ds, dr, [n // P] * P, dname, op)
            assert rc == 1 and st == [1] * P, (dname, op, rc, st)
            assert pico_amd.reduce_tree_wide([d.data_ptr() for d in ds], dr[0].data_ptr(), n, dname, op) == 1
            torch.cuda.synchronize()
            assert all((d.cpu().numpy() == 0xA5).all() for d in dr), (dname, op)
    L = pico_amd.lib()
    for d in (8, 9, 2, 3, 34):
        assert L.bine_widen(ds[0].data_ptr(), dr[0].data_ptr(), n, d, None) == 1
        assert L.bine_narrow(ds[0].data_ptr(), dr[0].data_ptr(), n, d, None) == 1

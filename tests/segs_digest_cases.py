"""The cases of tests/test_gpu_segs_digests.py and tools/segs_digests.py: every
entry of the segment family -- copy_segments, copy_shards, sumsq_segments,
clip_segments, adamw_segments and adamw_segments_dyn -- run on the smallest
shapes that reach each of its paths, and SHA-256 digests of what it left in
memory.  The fixture tests/golden/segs_digests.json holds the digests of the
commit before the family's dispatch was folded into one tile table; the kernels
are deterministic, so any later change of a bit shows.

Nothing here draws from a library's random generator: a buffer's content is a
closed-form integer hash of the element index (values()), and every buffer of
a case is a slice of ONE device arena whose base is 256-B aligned, so each
buffer's phase mod 16 B -- which the sums of squares' bits depend on -- is the
one the case asks for.  A digest covers the whole arena (inputs, outputs, the
0xA5 bytes between them), so a store outside a destination shows as well."""
import contextlib
import hashlib
import os

import numpy as np

TILE = 8192                      # floats per tile: 2048 16-B vectors, 32 KiB
PHASES = (0, 4, 8, 12)           # a buffer's address mod 16 B
COUNTS = (0, 1, 3, 5, TILE + 7, 2 * TILE)   # TILE + 7: a full tile, a guarded one and a tail
NSMALL, SMALL = 136, 7           # further segments: more than 128 non-empty ones in all
ESZ = {"float": 4, "double": 8, "float16": 2, "bfloat16": 2}
FILL = 0xA5
_M = np.uint64(0xFFFFFFFF)


def h32(n, salt):
    """a 32-bit hash of salt + 0 .. salt + n - 1 (uint64 arithmetic, masked)"""
    x = ((np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(2654435761)) & _M
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & _M
    x ^= x >> np.uint64(13)
    return x


def values(n, salt, kind, nonneg=False):
    """n elements of `kind` as bytes: multiples of 1/16 in [-7.9375, 7.9375]
    ([0, 15.875] if nonneg), exact in all four types; kind "bytes": n bytes"""
    h = h32(n, salt)
    if kind == "bytes":
        return (h & np.uint64(0xFF)).astype(np.uint8)
    f = ((h % np.uint64(255)).astype(np.int64) - (0 if nonneg else 127)).astype(np.float64) / 16.0
    if kind == "double":
        a = f
    elif kind == "float":
        a = f.astype(np.float32)
    elif kind == "float16":
        a = f.astype(np.float16)
    else:  # bfloat16: the upper half of the binary32 (8 significant bits suffice)
        a = (f.astype(np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    return a.view(np.uint8)


def seg_list(esz):
    """(count, phase) of the one segment list every entry walks; a phase that
    an element of esz bytes cannot stand on is rounded down to one it can"""
    segs = [(c, p - p % esz) for c in COUNTS for p in PHASES]
    return segs + [(SMALL, PHASES[i % 4] - PHASES[i % 4] % esz) for i in range(NSMALL)]


class Arena:
    """one device allocation; take() hands out byte offsets at a given phase
    mod 16 B, 64 or more FILL bytes between neighbours"""

    def __init__(self):
        self.size, self.parts = 256, []

    def take(self, nbytes, phase=0, data=None):
        off = self.size + phase
        if data is not None:
            assert len(data) == nbytes
            self.parts.append((off, data))
        self.size = (off + nbytes + 64 + 255) // 256 * 256
        return off

    def upload(self):
        import torch
        self.host = np.full(self.size, FILL, dtype=np.uint8)
        for off, data in self.parts:
            self.host[off:off + len(data)] = data
        self.t = torch.empty(self.size, dtype=torch.uint8, device="cuda:0")
        self.base = self.t.data_ptr()
        assert self.base % 256 == 0, "the arena's base fixes every phase mod 16 B"
        self.t.copy_(torch.from_numpy(self.host))
        torch.cuda.synchronize()

    def read(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy()

    def put(self, off, data):
        """bytes written after upload()"""
        import torch
        self.host[off:off + len(data)] = data
        self.t[off:off + len(data)].copy_(torch.from_numpy(np.ascontiguousarray(data)))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@contextlib.contextmanager
def sumsq_nt(value):
    """BINE_SUMSQ_NT = value (None: unset): the library reads it at every call"""
    saved = os.environ.pop("BINE_SUMSQ_NT", None)
    try:
        if value is not None:
            os.environ["BINE_SUMSQ_NT"] = value
        yield
    finally:
        os.environ.pop("BINE_SUMSQ_NT", None)
        if saved is not None:
            os.environ["BINE_SUMSQ_NT"] = saved


# ---- copy_segments ---------------------------------------------------------------------------

def _copy(pairs):
    """pairs: (bytes, source phase, destination phase)"""
    import pico_amd
    A = Arena()
    so = [A.take(b, sp, values(b, 7919 * k, "bytes")) for k, (b, sp, _) in enumerate(pairs)]
    do = [A.take(b, dp) for b, _, dp in pairs]
    A.upload()
    ptr = lambda off, b: A.base + off if b else None  # noqa: E731  (an empty segment may be NULL)
    pico_amd.copy_segments([ptr(o, p[0]) for o, p in zip(do, pairs)], [ptr(o, p[0]) for o, p in zip(so, pairs)],
                           [p[0] for p in pairs])
    got = A.read()
    for s, d, (b, _, _) in zip(so, do, pairs):
        assert got[d:d + b].tobytes() == A.host[s:s + b].tobytes()
    return {"arena": sha(got)}


def copy_coaligned():
    return _copy([(4 * c, p, p) for c, p in seg_list(4)])


def copy_shifted():
    """every source phase against destination phases 0, 1 and 5; 17 bytes: no
    vector (nvec == 0) wherever the destination does not stand on a boundary"""
    return _copy([(b, sp, dp) for b in (17, 4095, 4 * TILE + 1) for sp in range(16) for dp in (0, 1, 5)])


# ---- copy_shards -----------------------------------------------------------------------------

def copy_shards(dir):
    import pico_amd
    P, sizes = 3, [20, 4 * TILE + 4] + [12] * 130
    block = sum(sizes)
    A = Arena()
    data = [values(P * b, 104729 * (k + 1), "bytes") for k, b in enumerate(sizes)]
    fo = [A.take(P * b, PHASES[k % 4], None if dir else data[k]) for k, b in enumerate(sizes)]
    packed = np.zeros(P * block, dtype=np.uint8)
    poff = 0
    for k, b in enumerate(sizes):
        for j in range(P):
            packed[j * block + poff:j * block + poff + b] = data[k][j * b:(j + 1) * b]
        poff += b
    po = A.take(P * block, 0, packed if dir else None)
    A.upload()
    pico_amd.copy_shards(A.base + po, [A.base + o for o in fo], sizes, P, dir)
    got = A.read()
    assert got[po:po + P * block].tobytes() == packed.tobytes()
    for k, b in enumerate(sizes):
        assert got[fo[k]:fo[k] + P * b].tobytes() == data[k].tobytes()
    return {"arena": sha(got)}


# ---- sumsq_segments / clip_segments ----------------------------------------------------------

def _bucket(A, kind, salt):
    esz = ESZ[kind]
    segs = seg_list(esz)
    offs = [A.take(c * esz, p, values(c, salt + 65537 * k, kind)) for k, (c, p) in enumerate(segs)]
    return segs, offs


def sumsq(kind, nt):
    import pico_amd
    A = Arena()
    segs, offs = _bucket(A, kind, 11)
    n, cap = len(segs), 512
    out, scratch = A.take(8 * (n + 1), 0), A.take(8 * cap, 0)
    A.upload()
    addrs, counts = [A.base + o for o in offs], [c for c, _ in segs]
    assert pico_amd.plan_sumsq(addrs, counts, kind) <= cap
    with sumsq_nt(nt):
        pico_amd.sumsq_segments(addrs, dtype=kind, counts=counts, out=A.base + out, scratch=A.base + scratch,
                                scratch_doubles=cap)
    got = A.read()
    return {"out": sha(got[out:out + 8 * (n + 1)]), "arena": sha(got)}


def clip(kind, below_one, coef):
    """norm 100: max_norm 3 gives c = 3 / (100 + 1e-6) < 1, max_norm 1000 gives
    c == 1, after which every buffer is the input byte for byte"""
    import pico_amd
    A = Arena()
    segs, offs = _bucket(A, kind, 23)
    n2 = A.take(8, 0, np.array([1e4]).view(np.uint8))
    co = A.take(8, 8)
    A.upload()
    pico_amd.clip_segments([A.base + o for o in offs], A.base + n2, 3.0 if below_one else 1000.0, 1e-6, dtype=kind,
                           counts=[c for c, _ in segs], coef_out=A.base + co if coef else None)
    got = A.read()
    want = A.host.copy()
    if coef:
        c = 3.0 / (100.0 + 1e-6) if below_one else 1.0
        want[co:co + 8] = np.array([c]).view(np.uint8)
    same = got.tobytes() == want.tobytes()
    assert same == (not below_one)
    return {"arena": sha(got)}


def clip_coef_only(kind):
    """n == 0: one launch that stores the coefficient"""
    import pico_amd
    A = Arena()
    n2 = A.take(8, 0, np.array([1e4]).view(np.uint8))
    co = A.take(8, 8)
    A.upload()
    pico_amd.clip_segments([], A.base + n2, 3.0, 1e-6, dtype=kind, counts=[], coef_out=A.base + co)
    got = A.read()
    assert got[co:co + 8].view(np.float64)[0] == 3.0 / (100.0 + 1e-6)
    return {"arena": sha(got)}


# ---- adamw_segments / adamw_segments_dyn -----------------------------------------------------

HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1)
ELEM = ((TILE + 7, 0), (2 * TILE, 8))  # the segments whose m stands 4 B off: the element body


def adamw(gkind, okind, mode):
    """mode "plain": adamw_segments with a device coefficient; "dyn": the state
    of a taken step; "skip": the state of a skipped one -- nothing is stored"""
    import pico_amd
    A = Arena()
    segs = seg_list(4)
    gsz = ESZ[gkind]
    # g and pout stand on a 4-element boundary where p stands on a 16-B one
    po = [A.take(4 * c, p, values(c, 31 + 65537 * k, "float")) for k, (c, p) in enumerate(segs)]
    mo = [A.take(4 * c, (p + 4) % 16 if (c, p) in ELEM else p, values(c, 37 + 65537 * k, "float"))
          for k, (c, p) in enumerate(segs)]
    vo = [A.take(4 * c, p, values(c, 41 + 65537 * k, "float", nonneg=True)) for k, (c, p) in enumerate(segs)]
    go = [A.take(gsz * c, p * gsz // 4, values(c, 43 + 65537 * k, gkind)) for k, (c, p) in enumerate(segs)]
    oo = [A.take(ESZ[okind] * c, p * ESZ[okind] // 4) for c, p in segs] if okind else None
    gc = A.take(8, 0, np.array([0.75]).view(np.uint8))
    so = A.take(96, 8)
    A.upload()
    addr = lambda offs: None if offs is None else [A.base + o for o in offs]  # noqa: E731
    counts = [c for c, _ in segs]
    plan = pico_amd.plan_adamw(addr(po), addr(mo), addr(vo), addr(go), addr(oo), counts, gkind, okind or "float")
    assert [segs[int(e[1])] for e in plan if e[4]] == list(ELEM)
    assert len({int(e[0]) for e in plan}) == 3
    kw = dict(pout=addr(oo), gdtype=gkind, odtype=okind, counts=counts)
    if mode == "plain":
        pico_amd.adamw_segments(addr(po), addr(mo), addr(vo), addr(go), step=3, gcoef=A.base + gc,
                                grad_mul=1.0 / 1024, **HYPER, **kw)
    else:
        st = pico_amd.step_state_init(1024.0, 2, HYPER["beta1"], HYPER["beta2"])
        pico_amd.step_update_host(st, float("inf") if mode == "skip" else 1e9, max_norm=1.0, **HYPER)
        assert pico_amd.step_state_read(st)["skip"] == (1.0 if mode == "skip" else 0.0)
        A.put(so, st)
        pico_amd.adamw_segments_dyn(addr(po), addr(mo), addr(vo), addr(go), A.base + so, **kw)
    got = A.read()
    assert (got.tobytes() == A.host.tobytes()) == (mode == "skip")
    return {"arena": sha(got)}


# ---- the table -------------------------------------------------------------------------------

def _cases():
    c = {"copy_segments/coaligned": copy_coaligned, "copy_segments/shifted": copy_shifted}
    for d in (0, 1):
        c[f"copy_shards/dir{d}"] = lambda d=d: copy_shards(d)
    for kind in ESZ:
        for nt in (None, "1"):
            c[f"sumsq_segments/{kind}/nt_{nt or 'unset'}"] = lambda kind=kind, nt=nt: sumsq(kind, nt)
        for below, coef in ((True, True), (True, False), (False, True)):
            c[f"clip_segments/{kind}/{'below_one' if below else 'one'}/{'coef' if coef else 'no_coef'}"] = \
                lambda kind=kind, below=below, coef=coef: clip(kind, below, coef)
        c[f"clip_segments/{kind}/coef_only"] = lambda kind=kind: clip_coef_only(kind)
    for g in ("float", "bfloat16"):
        for o in (None, "bfloat16"):
            for mode in ("plain", "dyn", "skip"):
                entry = "adamw_segments" if mode == "plain" else "adamw_segments_dyn"
                c[f"{entry}/{g}/pout_{o or 'none'}/{mode}"] = lambda g=g, o=o, mode=mode: adamw(g, o, mode)
    return c


CASES = _cases()

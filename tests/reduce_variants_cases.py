"""The shapes of tests/test_gpu_reduce_variants.py and tools/reduce_env_check.py
(test infrastructure), with a host model of k_reduce's index arithmetic that
says what each shape reaches (proved on the CPU by
tests/test_reduce_variants_cases.py).

k_reduce<T, OP, U, NT> (pico_amd/csrc/kernels.hip): `blocks` workgroups of 256
lanes; workgroup w, lane l starts at vector base = w * tile + l, tile = 256 * U.
The full-tile loop runs while base + (U - 1) * 256 < nvec, handles the U
vectors base + u * 256 without bounds checks and advances base by blocks *
tile.  The guarded loop after it ("the partial tile") handles the vectors
base + u * 256 < nvec from the base the loop left.  blocks = min(tiles, cap),
cap = the tuning's maxblocks or 16384.

Terms used below, per workgroup:
  trip      one pass of the full-tile loop by a lane
  (b)       a lane takes two or more trips
  (c)       a lane leaves the loop, after one trip or more, at a tile that
            begins below nvec (its workgroup ends on a partial tile); U >= 2:
            it then writes one vector or more in the guarded loop.  U = 1: the
            loop's condition is base < nvec, so the guarded loop never writes
            (asserted by the CPU test) and the partial tile is taken by the
            loop itself, by the lanes that reach it
  (d)       every lane leaves the loop, after one trip or more, with base at
            or past nvec: the guarded loop writes nothing
  (e)       some lanes take a tile as a trip while other lanes of the same
            workgroup leave the loop at that tile (U >= 2: and write there
            in the guarded loop)

Element counts: phase 0 puts every operand on a 16-B boundary, n = nvec
vectors exactly; phase 1 puts every operand one element past a 16-B boundary:
a head of 16 / esz - 1 elements, nvec vectors and a tail of 1 .. 16 / esz - 1
elements (16-byte elements: neither head nor tail)."""
import numpy as np

KBLOCK = 256
US = (1, 2, 4, 8)                 # k_reduce's U for float SUM
NTS = (0, 1, 2, 3, 4, 5, 7)       # ... and its NT masks (reduce_t's NTSW)
DEFAULT_U = 4
DEFAULT_CAP = 16384               # kDefaultMaxBlocks
CAPS = (0, 1, 3)                  # 0: the default cap
PHASES = (0, 1)
SCALAR_ABOVE = 4096               # operands not co-aligned mod 16 B: k_reduce_scalar above this count
GUARD = 0xA5
GUARD_BYTES = 64


def tile(U):
    return KBLOCK * U


def multi(U):
    """7 whole tiles and (U - 1) * 256 + 100 vectors: with a cap of 2 or 3 workgroups (b) .. (e)
    all happen; lanes below 100 take tile 7 as a trip, the others in the guarded loop"""
    return 7 * tile(U) + KBLOCK * (U - 1) + 100


def partial(U):
    """4 whole tiles and 100 vectors: with a cap of 3, workgroup 1 ends on a partial tile that
    (U >= 2) no lane takes as a trip"""
    return 4 * tile(U) + 100


def counts(U):
    """the vector counts of the float SUM matrix: the edges around one tile and the two multi-trip shapes"""
    t = tile(U)
    return (0, 1, t - 1, t, t + 1, partial(U), multi(U))


def blocks_of(nvec, U, cap):
    """run_reduce's grid"""
    if nvec == 0:
        return 1
    tiles = (nvec + tile(U) - 1) // tile(U)
    return min(tiles, cap if cap > 0 else DEFAULT_CAP)


def split(addr, n, esz):
    """vec_split: (head elements, whole vectors) of n elements of esz bytes at address addr"""
    head = min(((16 - (addr & 15)) & 15) // esz, n)
    return head, (n - head) // (16 // esz)


def tail_of(nvec, esz):
    per = 16 // esz
    return 1 + nvec % (per - 1) if per > 1 else 0


def elements(nvec, esz, phase):
    """the element count that gives nvec vectors at the phase"""
    per = 16 // esz
    return nvec * per if phase == 0 else (per - 1) + nvec * per + tail_of(nvec, esz)


def walk(nvec, U, blocks):
    """k_reduce's loops restated: per workgroup, per lane, (the trips' vectors, the guarded loop's
    vectors, base as the loop left it)"""
    t, stride = tile(U), blocks * tile(U)
    out = []
    for wg in range(blocks):
        lanes = []
        for lane in range(KBLOCK):
            base = wg * t + lane
            trips = []
            while base + (U - 1) * KBLOCK < nvec:
                trips.append([base + u * KBLOCK for u in range(U)])
                base += stride
            guarded = [base + u * KBLOCK for u in range(U) if base + u * KBLOCK < nvec]
            lanes.append((trips, guarded, base))
        out.append(lanes)
    return out


def written(nvec, U, blocks):
    """how often each vector is written; index nvec counts every write at or past nvec"""
    w = np.zeros(nvec + 1, dtype=np.int64)
    for lanes in walk(nvec, U, blocks):
        for trips, guarded, _ in lanes:
            for v in [x for trip in trips for x in trip] + guarded:
                w[min(v, nvec)] += 1
    return w


def reaches(nvec, U, blocks):
    """which of (b) .. (e) the launch reaches, as a set of letters"""
    t = tile(U)
    got = set()
    for lanes in walk(nvec, U, blocks):
        if any(len(trips) >= 2 for trips, _, _ in lanes):
            got.add("b")
        if all(trips and base >= nvec for trips, _, base in lanes):
            got.add("d")
        tripped = {x[0] // t for trips, _, _ in lanes for x in trips}      # the tiles taken as trips
        for lane, (trips, guarded, base) in enumerate(lanes):
            at = (base - lane) // t                                          # the tile the lane left the loop at
            if trips and at * t < nvec and (guarded or U == 1):
                got.add("c")
                if at in tripped:
                    got.add("e")
    return got


# ---- the arena: operands and output between guard bytes ------------------------------------------

def layout(n, esz, phases):
    """byte offsets of len(phases) regions of n elements, each `phase` elements past a 16-B
    boundary with GUARD_BYTES or more of guard on either side, and the arena's size"""
    offs, o = [], 0
    for ph in phases:
        offs.append(o + GUARD_BYTES + ph * esz)
        o = (offs[-1] + n * esz + GUARD_BYTES + 63) & ~63
    return offs, o


class Arena:
    """a, b and out (phases: elements past a 16-B boundary, in that order) in one byte buffer of
    guard bytes.  A call leaves the arena as expected(result, inplace): the result's bytes in out
    (in b when out aliases b), every other byte -- a, the out-of-place b, every guard byte, out
    when it is not used -- as it was."""

    NAMES = ("a", "b", "out")

    def __init__(self, a, b, phases=(0, 0, 0)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.size == b.size
        self.n, self.esz = a.size, a.dtype.itemsize
        self.off, size = layout(self.n, self.esz, phases)
        self.init = np.full(size, GUARD, dtype=np.uint8)
        for x, o in ((a, self.off[0]), (b, self.off[1])):
            self.init[o:o + x.nbytes] = x.view(np.uint8).reshape(-1)
        self.work = self.dev_init = None

    def expected(self, result, inplace):
        img = self.init.copy()
        raw = np.ascontiguousarray(result).view(np.uint8).reshape(-1)
        assert raw.size == self.n * self.esz
        o = self.off[1 if inplace else 2]
        img[o:o + raw.size] = raw
        return img

    def where(self, byte):
        """names a byte of the arena"""
        for name, o in zip(self.NAMES, self.off):
            if o <= byte < o + self.n * self.esz:
                return f"{name}[{(byte - o) // self.esz}]"
            if o - GUARD_BYTES <= byte < o:
                return f"{o - byte} bytes before {name}"
            if 0 <= byte - o - self.n * self.esz < GUARD_BYTES:
                return f"{byte - o - self.n * self.esz} bytes past {name}"
        return f"guard byte {byte}"

    # the device side (torch is imported here: the table itself needs no GPU)
    def upload(self, img=None):
        import torch
        t = torch.from_numpy(self.init if img is None else img).to("cuda:0")
        if img is None:
            self.dev_init, self.work = t, torch.empty_like(t)
            assert self.work.data_ptr() % 64 == 0
        return t

    def reset(self):
        self.work.copy_(self.dev_init)

    def ptr(self, k):
        return self.work.data_ptr() + self.off[k]

    def matches(self, dev_img):
        import torch
        return bool(torch.equal(self.work, dev_img))

    def first_difference(self, img, ignore=None, same=None):
        """None, or the first byte at which the device's arena differs from the host image
        (ignore: a mask of bytes left out; same(got, want): the comparison's own notion of equal
        for a whole region, used for out and b)"""
        got = self.work.cpu().numpy()
        if same is not None:
            for o in self.off[1:]:
                s = slice(o, o + self.n * self.esz)
                if same(got[s], img[s]):
                    got[s] = img[s]
        ne = got != img
        if ignore is not None:
            ne &= ~ignore
        idx = np.flatnonzero(ne)
        return None if idx.size == 0 else f"byte {idx[0]} ({self.where(int(idx[0]))}), {idx.size} bytes differ"


def padding_mask(arena, nd, region):
    """the bytes of the region (1: b, 2: out) that are padding of MPI's pair types (not part of
    the type map: oracle.canonical)"""
    nd = np.dtype(nd)
    mask = np.zeros(arena.init.size, dtype=bool)
    if not nd.names:
        return mask
    pad = np.ones(nd.itemsize, dtype=bool)
    for name in nd.names:
        f, o = nd.fields[name][0], nd.fields[name][1]
        pad[o:o + f.itemsize] = False
    o = arena.off[region]
    mask[o:o + arena.n * nd.itemsize] = np.tile(pad, arena.n)
    return mask

"""The bits of the segment family, pinned: every case of
tests/segs_digest_cases.py -- copy_segments, copy_shards, sumsq_segments,
clip_segments, adamw_segments and adamw_segments_dyn on the smallest shapes that
reach every path of their kernels -- must leave the bytes whose SHA-256 digests
tests/golden/segs_digests.json holds (recorded by tools/segs_digests.py before
the family's dispatch became one tile table, one search and one fill).  For the
sums of squares the digest of the raw doubles is kept beside the arena's."""
import json
import os

import pytest

import segs_digest_cases as C

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segs_digests.json")


@pytest.fixture(scope="module")
def golden():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(C.CASES)


@pytest.mark.parametrize("name", list(C.CASES))
def test_digest(golden, name):
    got = C.CASES[name]()
    assert name in golden, f"{name}: not in the fixture"
    assert got == golden[name], name

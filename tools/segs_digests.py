#!/usr/bin/env python3
"""Record tests/golden/segs_digests.json: the digests of every case of
tests/segs_digest_cases.py, as the library of THIS tree computes them on the GPU.

    python tools/segs_digests.py [out.json]

The fixture is recorded once, on the commit whose bits are to be kept (the Python
API the cases use must be that commit's too), and compared by
tests/test_gpu_segs_digests.py on every later one."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import segs_digest_cases as C  # noqa: E402


def main(argv):
    out = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "segs_digests.json")
    digests = {}
    for name, run in C.CASES.items():
        digests[name] = run()
        print(name, digests[name], flush=True)
    with open(out, "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} cases -> {out}")


if __name__ == "__main__":
    main(sys.argv)

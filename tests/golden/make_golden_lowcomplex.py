"""Rewrites tests/golden/lowcomplex.json: digests of the oracle's results on the low-complexity cases (tests/lowcomplex_cases.py) and of the
generator's genomes.  Digests only; run from the repository root: python tests/golden/make_golden_lowcomplex.py"""
import json
import os
import sys
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import lowcomplex_cases as lc  # noqa: E402
from common import arr_digest  # noqa: E402
from test_lowcomplex import digests, GOLD  # noqa: E402

out = {"genome": {m: arr_digest(lc.genome(60000, 1, m)) for m in ("mixed", "dense")}, "cases": {}}
for name in sorted(lc.CASES):
    wo, fo, bo = lc.oracle(name)
    print(name, lc.measure(name, wo), flush=True)
    out["cases"][name] = digests(name)
with open(GOLD, "w") as f:
    json.dump(out, f, indent=0, sort_keys=True)

"""python feas_need_cfg2.py <audit file> <piles>: the first piles of config 2 (tests/scale_cases.py: bench.py's data set, k = 14) on the 1-lane
emulation with the audit aid of the stretch-feasibility filter on (DACC_EMUL_FEASNEED), once with the filter and once without it
(DACC_FEAS_NEED=0); prints one JSON line: the audit's totals of either run and whether the two runs returned the same windows, fragments and
bases.  A process of its own because the emulation opens the audit file once per process (tests/test_feas_need.py)."""
import json
import os
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_root, os.path.join(_root, "oracle")]

import pyoracle
from daccord_amd._structs import default_params
from scale_cases import CASES, make_case
from feas_need_cases import AUDIT, read_audit


def main(argv):
    audit, npiles = argv[0], int(argv[1])
    os.environ["DACC_EMUL_FEASNEED"] = audit
    import emul_lib
    from common import windows_equal, frags_equal
    case = dict(CASES["cfg2"]); case["npiles"] = npiles
    d, ovl, piles, sel = make_case(case, pyoracle.pile_select)
    p = default_params(**case["params"][0])
    out, runs, prev = {}, {}, dict(zip(AUDIT, [0] * len(AUDIT)))
    for need in ("1", "0"):
        os.environ["DACC_FEAS_NEED"] = need
        E = emul_lib.Emul(p); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
        fe, be = E.run(sel, ovl, d.trace)
        runs[need] = (E.windows(), fe, be)
        now = read_audit(audit)
        out["audit_" + need] = {n: now[n] - prev[n] for n in AUDIT}
        prev = now
        del E
    (w1, f1, b1), (w0, f0, b0) = runs["1"], runs["0"]
    out["windows"] = len(w1)
    out["on_equals_off"] = len(windows_equal(w0, w1)) == 0 and bool(frags_equal(f0, b0, f1, b1)) and bytes(b1) == bytes(b0)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])

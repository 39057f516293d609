"""Shapes of the stretch-feasibility tests (tests/test_feas_pipeline.py on the CPU, tests/test_gpu_feas_pipeline.py on the device): a few piles of
2 kb reads at 20x and at 54x, k = 8 and k = 14, on random sequence and on the low-complexity genomes of tests/lowcomplex_cases.py (nodes with
several instances).  Between them they reach every situation of computeStretchFeasLanes' unit order, task rounds and node pipeline that the
tests list; the emulation's counters (DACC_EMUL_FEASCASES) say so and the CPU test asserts it.

The oracle's result of a case is computed once per process, shared and never modified."""
import os
import sys

if __name__ == "__main__":      # run as the script of a case (see _main): the paths tests/conftest.py sets for the suite
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle")]

import pyoracle
import lowcomplex_cases as lc
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData

_S20 = dict(genome_len=3000, nreads=30, read_len=2000, seed=11)          # 30 reads x 2 kb at 20x
_D54 = dict(genome_len=2200, nreads=60, read_len=2000, seed=4)           # 60 reads x 2 kb at 54x

# name -> (SynthData arguments, (mode, seed) of a low-complexity genome or None, parameters, slice of the selected piles)
CASES = {
    "s20_k14":  (_S20, None, dict(k=14), (0, 6)),
    "s20_k8":   (_S20, None, dict(k=8), (0, 6)),
    "lc20_k8":  (_S20, ("mixed", 1), dict(k=8), (0, 6)),
    "lc20_k14": (_S20, ("dense", 1), dict(k=14), (0, 6)),
    # two piles each, for the 64-lane emulation; "pin" is also the record-level pin (tests/golden/feas_pipeline_trav.txt)
    "pin":      (_S20, ("mixed", 1), dict(k=8), (0, 2)),
    "lcd_k14s": (_S20, ("dense", 1), dict(k=14), (0, 2)),
    "d54_k14":  (_D54, None, dict(k=14), (28, 31)),
    "d54_k8":   (_D54, ("mixed", 2), dict(k=8), (28, 30)),
}
LANES64 = ("pin", "lcd_k14s")      # the cases that also run on the 64-lane emulation

# columns of a line of the emulation's DACC_EMUL_FEASCASES file (fast_window.hpp: struct FeasCases), one line per traversal
COLUMNS = ("tier", "nu", "ncu", "ntask", "empty_first", "empty_mid", "empty_last", "start_at_round", "start_at_round_end", "spans_rounds", "rounds", "lenmask", "maxlen",
           "at_clamp", "past_clamp", "multi", "fail0", "fail1", "faillast", "nodes", "nwF", "nwR")

_data = {}
_oracle = {}


def params(name):
    return default_params(**CASES[name][2])


def shape(name):
    """(data set, selected overlaps, the case's piles)"""
    kw, lcg, _, (a, b) = CASES[name]
    key = (tuple(sorted(kw.items())), lcg)
    if key not in _data:
        g = lc.genome(kw["genome_len"], lcg[1], lcg[0]) if lcg else None
        d = SynthData(genome=g, **kw)
        _data[key] = (d,) + tuple(pyoracle.pile_select(d.ovl, d.piles))
    d, ovl, piles = _data[key]
    return d, ovl, piles[a:b]


def oracle(name, nthreads=8):
    """(windows, fragments, bases) of the oracle"""
    if name not in _oracle:
        d, ovl, sel = shape(name)
        O = pyoracle.Oracle(params(name)); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
        fo, bo = O.run(sel, ovl, d.trace, nthreads=nthreads, want_windows=True)
        _oracle[name] = (O.windows(), fo, bo)
    return _oracle[name]


def _main(argv):
    """python feas_cases.py <case> <lanes> <prefix>: one emulation run in a process of its own with the emulation's trace files on
    (<prefix>.trav: DACC_EMUL_TRAV, <prefix>.cases: DACC_EMUL_FEASCASES -- both are opened once per process, at the first traversal),
    compared with the live oracle; prints one JSON line"""
    import json
    case, lanes, prefix = argv[0], int(argv[1]), argv[2]
    os.environ["DACC_EMUL_TRAV"] = prefix + ".trav"
    os.environ["DACC_EMUL_FEASCASES"] = prefix + ".cases"
    import emul_lib
    from common import windows_equal, frags_equal
    d, ovl, sel = shape(case)
    E = emul_lib.Emul(params(case), lanes=lanes); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fe, be = E.run(sel, ovl, d.trace)
    wo, fo, bo = oracle(case)
    bad = windows_equal(wo, E.windows())
    print(json.dumps({"windows": len(wo), "bad_windows": len(bad), "frags_equal": bool(frags_equal(fo, bo, fe, be)), "fasta_equal": pyoracle.fasta(fe, be) == pyoracle.fasta(fo, bo),
                      "counts": list(E.counts()), "tier0": E.count_tier0(), "tier7": E.count_tier7(), "tier10": E.count_tier10()}))


if __name__ == "__main__":
    _main(sys.argv[1:])

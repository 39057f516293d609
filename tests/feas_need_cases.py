"""Shapes of the tests of the stretch-feasibility filter (computeStretchFeasLanes computes only the (stretch, direction, start position)
triples the enumerations of the traversal can read; DACC_FEAS_NEED=0 computes all of them): tests/test_feas_need.py on the host emulation,
tests/test_gpu_feas_need.py on the device.  The smallest shapes of the existing generators (tests/feas_cases.py, tests/lowcomplex_cases.py,
tests/edge_cases.py) at which a rule of the filter can go wrong:

  s20_k14   random sequence at k = 14: first and last k-mer candidates strictly inside a stretch
  s20_k8    k = 8: H - k is large, reverse units far from the last k-mer are read
  lc_k8     low-complexity sequence, k = 8: cyclic graphs (the distances relax round a loop), nodes with several instances
  lc_k14    dense low-complexity sequence, k = 14: a first and a last candidate inside the same stretch (middle pieces, pairs on their exact
            stretch set)
  w24_k14   w = 24 at k = 14: H = (lmax+1)/2 <= k, no reverse path is extended beyond the roots' extensions
  ff0       maxfilterfreq = 0: every window is decided at filter frequency 0, the densest graphs
  w96_k8    wide windows (w = 96): two-word masks, start positions up to 127
  d54_k14   a deep pile (54x): the deep chain

The audit aid of the emulation (DACC_EMUL_FEASNEED, fast_window.hpp: struct FeasNeedAudit) says what the filter left out of a run, which
situations the run went through and how often an enumeration asked for something that was left out.  Data sets and oracle results are computed
once per process, shared and never modified."""
import os
import sys

if __name__ == "__main__":      # run as the script of a case (see _main): the paths tests/conftest.py sets for the suite
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle")]

import pyoracle
import feas_cases as fc
import lowcomplex_cases as lc
import edge_cases as ec
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData

# name -> (data: ("feas", SynthData arguments, low-complexity genome or None) | ("edge", case of tests/edge_cases.py), parameters, slice of the piles)
CASES = {
    "s20_k14": (("feas", fc._S20, None), dict(k=14), (0, 2)),
    "s20_k8":  (("feas", fc._S20, None), dict(k=8), (0, 1)),
    "lc_k8":   (("feas", fc._S20, ("mixed", 1)), dict(k=8), (0, 1)),
    "lc_k14":  (("feas", fc._S20, ("dense", 1)), dict(k=14), (0, 1)),
    "w24_k14": (("feas", fc._S20, None), dict(k=14, w=24, a=6), (0, 1)),
    "ff0":     (("edge", "maxfilterfreq0"), dict(k=8, maxfilterfreq=0), (0, 1)),
    "w96_k8":  (("feas", fc._S20, None), dict(k=8, w=96, a=24), (0, 1)),
    "d54_k14": (("feas", fc._D54, None), dict(k=14), (28, 29)),
}
LANES64 = ("lc_k8", "w24_k14")      # the cases that also run on the 64-lane emulation

# columns of the line the audit aid writes (running totals of a process)
AUDIT = ("traversals", "units_all", "tasks_all", "units_kept", "tasks_kept", "rec_f", "rec_r", "probes_f", "probes_r", "links_r",
         "first_inside", "last_inside", "middle_pieces", "h_le_k", "relax_passes")

_data = {}
_oracle = {}


def params(name):
    return default_params(**CASES[name][1])


def shape(name):
    """(data set, selected overlaps, the case's piles)"""
    src, _, (a, b) = CASES[name]
    if src[0] == "edge":
        d, ovl, piles = ec.data(src[1])
        return d, ovl, piles[a:b]
    kw, lcg = src[1], src[2]
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
        fo, bo = O.run(sel, ovl, d.trace, trace_bytes=getattr(d, "trace_bytes", 1), nthreads=nthreads, want_windows=True)
        _oracle[name] = (O.windows(), fo, bo)
    return _oracle[name]


def read_audit(path):
    v = [int(x) for x in open(path).read().split()]
    assert len(v) == len(AUDIT), v
    return dict(zip(AUDIT, v))


def _main(argv):
    """python feas_need_cases.py <lanes> <audit file> <case> ...: the cases on the emulation in a process of its own (the audit file is opened
    once per process), each with the filter and then without it, both compared with the live oracle and with each other; prints one JSON line
    per case with the audit's totals of the filtered run"""
    import json
    lanes, audit = int(argv[0]), argv[1]
    os.environ["DACC_EMUL_FEASNEED"] = audit
    import emul_lib
    from common import windows_equal, frags_equal
    prev = dict(zip(AUDIT, [0] * len(AUDIT)))
    for case in argv[2:]:
        d, ovl, sel = shape(case)
        wo, fo, bo = oracle(case)
        out = {"case": case, "windows": len(wo), "ff0": int(((wo["status"] == 1) & (wo["filterfreq"] == 0)).sum()), "wide": int(params(case).w) > 64}
        runs = {}
        for need in ("1", "0"):
            os.environ["DACC_FEAS_NEED"] = need
            E = emul_lib.Emul(params(case), lanes=lanes); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
            fe, be = E.run(sel, ovl, d.trace, trace_bytes=getattr(d, "trace_bytes", 1))
            we = E.windows()
            runs[need] = (we, fe, be)
            out["bad_windows_" + need] = len(windows_equal(wo, we))
            out["equal_" + need] = bool(frags_equal(fo, bo, fe, be)) and bytes(be) == bytes(bo) and pyoracle.fasta(fe, be) == pyoracle.fasta(fo, bo)
            out["fast_windows_" + need] = len(wo) - E.counts()[3]      # finished by the tiers, not by the generic engine
            now = read_audit(audit)
            out["audit_" + need] = {n: now[n] - prev[n] for n in AUDIT}
            prev = now
            del E
        (w1, f1, b1), (w0, f0, b0) = runs["1"], runs["0"]
        out["on_equals_off"] = len(windows_equal(w0, w1)) == 0 and bool(frags_equal(f0, b0, f1, b1)) and bytes(b1) == bytes(b0)
        print(json.dumps(out), flush=True)
    os.environ.pop("DACC_FEAS_NEED", None)


if __name__ == "__main__":
    _main(sys.argv[1:])

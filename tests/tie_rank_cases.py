"""python tie_rank_cases.py <lanes> <stats file> cfg2:<first>:<npiles> | <case of feas_need_cases.py> ...: the inputs of tests/test_tie_rank.py on the
host emulation, in a process of its own (the emulation opens the DACC_EMUL_STATS file once per process), each with the lane-parallel tie rank
(the default) and then with DACC_TIE_FAST=0, both compared with the live oracle and with each other.  Prints one JSON line per input:

  windows, bad_windows_<1|0>, equal_<1|0>   windows of the oracle, windows that differ from it, fragments / bases / FASTA equal to it
  on_equals_off                             the two runs returned the same windows array (every byte), fragments and bases
  ties_<1|0>, exact_<1|0>                   windows with a traversal whose kept candidates share a weight (column 21 of the statistics line);
                                            windows with a traversal that took lane 0's two heaps AFTER the lane-parallel rank (column 32)
  state                                     of the default run (1 lane only): per-window status / filterfreq / k / conslen (SHA-256); the tier
                                            counts; the overflow flags: every over() of every tier in the order it happened (DACC_EMUL_OVER
                                            lines without their source line number: tier, bits, the sizes of the graph at that moment; count,
                                            SHA-256 and a histogram tier -> bits -> count), the flags each slot's main tier handed on with
                                            (emul_reasons_tier: hand-over reason codes and one counter per flag bit) and the (window, flags)
                                            list of the generic engine (emul_generic_list).  tests/golden/tie_rank_state.json records it of the
                                            commit before the change (--record writes it from the library DACC_EMUL_LIB names)"""
import collections
import ctypes as C
import hashlib
import json
import os
import re
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_root, os.path.join(_root, "oracle")]

import numpy as np
import pyoracle
from daccord_amd._structs import default_params
from scale_cases import CASES, make_case
import feas_need_cases as fn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tie_rank_state.json")
NSTAT = 33      # FastStats::N


def shape(name):
    """(data, selected overlaps, piles, parameters) of an input"""
    if name.startswith("cfg2:"):
        _, first, npiles = name.split(":")
        case = dict(CASES["cfg2"]); case["first"] = int(first); case["npiles"] = int(npiles)
        d, ovl, piles, sel = make_case(case, pyoracle.pile_select)
        return d, ovl, sel, default_params(**case["params"][0])
    d, ovl, sel = fn.shape(name)
    return d, ovl, sel, fn.params(name)


class Stderr:
    """file descriptor 2 goes to `path` (appended) inside the block: the emulation's DACC_EMUL_OVER lines are written by C code"""
    def __init__(self, path):
        self.path = path

    def __enter__(self):
        sys.stderr.flush()
        self.saved = os.dup(2)
        fd = os.open(self.path, os.O_WRONLY | os.O_CREAT | os.O_APPEND, 0o644)
        os.dup2(fd, 2); os.close(fd)

    def __exit__(self, *a):
        sys.stderr.flush()
        os.dup2(self.saved, 2); os.close(self.saved)


_OVER = re.compile(r"^\[over\] tier maxs=(\d+) line \d+ bits (0x[0-9a-f]+) (.*)$")


def over_events(path, skip):
    """the over() calls behind the first `skip` lines of the file: (count, SHA-256 of tier / bits / sizes in order, {tier: {bits: count}}, lines read)"""
    lines = open(path).read().splitlines()[skip:]
    h = hashlib.sha256(); hist = collections.defaultdict(collections.Counter); n = 0
    for l in lines:
        m = _OVER.match(l)
        assert m, l
        h.update(("%s %s %s\n" % m.groups()).encode()); hist[m.group(1)][m.group(2)] += 1; n += 1
    return n, h.hexdigest(), {t: dict(sorted(c.items())) for t, c in sorted(hist.items())}, len(lines)


def state(E, w, over):
    h = hashlib.sha256()
    for f in ("status", "filterfreq", "k", "conslen"):
        h.update(np.ascontiguousarray(w[f]).tobytes())
    E.L.emul_generic_list.restype = C.c_uint64; E.L.emul_generic_list.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    n = E.L.emul_generic_list(E.h, None, 0); g = np.zeros(n, np.uint64)
    E.L.emul_generic_list(E.h, g.ctypes.data_as(C.c_void_p), n)
    E.L.emul_reasons_tier.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    handed = []
    for t in range(3):
        r = (C.c_uint64 * 64)(); fb = (C.c_uint64 * 24)()
        E.L.emul_reasons_tier(E.h, t, r, fb)
        handed.append({"reasons": {str(i): int(x) for i, x in enumerate(r) if x}, "flag_bits": {str(i): int(x) for i, x in enumerate(fb) if x}})
    return {"sha256": h.hexdigest(), "counts": list(E.counts()), "tier0": E.count_tier0(), "tier7": E.count_tier7(), "tier10": E.count_tier10(),
            "over_events": over[0], "over_sha256": over[1], "over_bits": over[2], "handed_on": handed, "generic": [[int(a), int(b)] for a, b in g.reshape(-1, 2)]}


def read_stats(path, skip, lanes):
    """(windows with a tie, windows on the exact route after the fast one, lines read) of the statistics lines behind the first `skip`:
    one line per window and tier that ran it, written by every lane of the emulated wavefront"""
    rows = [l.split() for l in open(path).read().splitlines()][skip:]
    assert all(len(r) == 1 + NSTAT for r in rows)
    return sum(int(r[1 + 21]) > 0 for r in rows) // lanes, sum(int(r[1 + 32]) > 0 for r in rows) // lanes, len(rows)


def main(argv):
    record = "--record" in argv
    argv = [a for a in argv if a != "--record"]
    lanes, stats = int(argv[0]), argv[1]
    os.environ["DACC_EMUL_STATS"] = stats
    overfile = stats + ".over"      # 1 lane: every over() call reports itself (the emulation reads the switch once per process)
    if lanes == 1:
        os.environ["DACC_EMUL_OVER"] = "1"
    open(overfile, "w").close()
    oseen = 0
    import emul_lib
    from common import windows_equal, frags_equal
    gold = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
    seen = 0
    for name in argv[2:]:
        d, ovl, sel, p = shape(name)
        tb = getattr(d, "trace_bytes", 1)
        if record:
            E = emul_lib.Emul(p, lanes=lanes); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
            with Stderr(overfile):
                E.run(sel, ovl, d.trace, trace_bytes=tb)
            ov = over_events(overfile, oseen); oseen += ov[3]
            gold[name] = state(E, E.windows(), ov)
            continue
        O = pyoracle.Oracle(p); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
        fo, bo = O.run(sel, ovl, d.trace, trace_bytes=tb, nthreads=8, want_windows=True)
        wo = O.windows()
        out = {"case": name, "windows": len(wo)}
        runs = {}
        for fast in ("1", "0"):
            os.environ["DACC_TIE_FAST"] = fast
            E = emul_lib.Emul(p, lanes=lanes); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
            with Stderr(overfile):
                fe, be = E.run(sel, ovl, d.trace, trace_bytes=tb)
            we = E.windows()
            ov = over_events(overfile, oseen); oseen += ov[3]
            runs[fast] = (we, fe, be)
            out["bad_windows_" + fast] = len(windows_equal(wo, we))
            out["equal_" + fast] = bool(frags_equal(fo, bo, fe, be)) and bytes(be) == bytes(bo) and pyoracle.fasta(fe, be) == pyoracle.fasta(fo, bo)
            out["ties_" + fast], out["exact_" + fast], n = read_stats(stats, seen, lanes)
            seen += n
            if fast == "1":
                out["state"] = state(E, we, ov)
            del E
        os.environ.pop("DACC_TIE_FAST", None)
        (w1, f1, b1), (w0, f0, b0) = runs["1"], runs["0"]
        out["on_equals_off"] = w1.tobytes() == w0.tobytes() and bool(frags_equal(f0, b0, f1, b1)) and bytes(b1) == bytes(b0)
        print(json.dumps(out), flush=True)
    if record:
        json.dump(gold, open(GOLDEN, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv[1:])

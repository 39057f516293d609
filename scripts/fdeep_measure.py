"""The full-depth stage (k_window_fast<18>) on one pile of tests/fdeep_cases.py, one process per library (DACC_LIB selects it; a process cannot change
libraries): one submit and `steps` resident passes, one JSON line with the times of every pass (device events of dacc_timing), the trailing stages'
counters and a digest of the FASTA.  A library whose dacc_timing ends at 192 bytes leaves the full-depth fields zero.
usage: [DACC_LIB=<lib.so>] python scripts/fdeep_measure.py <shape: Q | R> <k> [steps=3] [maxalign]"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import fdeep_cases as fc
from daccord_amd import engine
from daccord_amd._structs import default_params


def main():
    name, k = sys.argv[1], int(sys.argv[2])
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    kw = dict(k=k)
    if len(sys.argv) > 4:
        kw["maxalign"] = int(sys.argv[4])
    d, ovl, sel = fc.shape(name)
    E = engine.Engine(default_params(**kw)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fr, ba = E(sel, ovl, d.trace)
    t = E.timing_full()
    first = dict(window_ms=round(t.window_ms, 2), xdeep_ms=round(t.xdeep_ms, 2), fdeep_ms=round(t.fdeep_ms, 2), total_ms=round(t.total_ms, 2))
    win, xms, fms = [], [], []
    for _ in range(steps):
        E.rerun(); fr, ba = E.collect(); t = E.timing_full()
        win.append(round(t.window_ms, 2)); xms.append(round(t.xdeep_ms, 2)); fms.append(round(t.fdeep_ms, 2))
    wx = E.debug_windows()
    print(json.dumps({"lib": os.path.basename(os.environ.get("DACC_LIB", "libdaccord_hip.so")), "shape": name, "k": k, "maxalign": kw.get("maxalign"), "nwindows": int(t.nwindows),
                      "strings": [int(wx["mao"].min()), int(wx["mao"].max())], "submit": first, "window_ms": win, "xdeep_ms": xms, "fdeep_ms": fms,
                      "last": [int(t.last_windows), int(t.last_out)], "vdeep": [int(t.vdeep_windows), int(t.vdeep_out)], "xdeep": [int(t.xdeep_windows), int(t.xdeep_out)],
                      "fdeep": [int(t.fdeep_windows), int(t.fdeep_out)], "tier_out": [int(x) for x in t.tier_out], "bases": len(ba),
                      "sha": hashlib.sha256(engine.fasta(fr, ba).encode()).hexdigest()[:16]}), flush=True)
    E.close()


main()

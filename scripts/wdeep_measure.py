"""The wide deep stage (k_window_fast<19>) on the shapes of tests/wdeep_cases.py and on a throughput shape, one process per library (DACC_LIB selects it; a
process cannot change libraries): one submit and `steps` resident passes, one JSON line with the times of every pass (device events of dacc_timing), the
trailing stages' counters and a digest of the FASTA.  A library whose dacc_timing ends at 208 bytes leaves the wide deep fields zero.
Shape T: the data of shape D with the overlaps of eight A reads (aread_range = (996, 1004)) at WD's parameters, eight piles of windows of several hundred strings.
usage: [DACC_LIB=<lib.so>] python scripts/wdeep_measure.py <shape: WD | WM | ... | T> [steps=3]"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import pyoracle
import vdeep_cases as vc
import wdeep_cases as wc
from daccord_amd import engine
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData


def main():
    name = sys.argv[1]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    if name == "T":
        d = SynthData(**dict(vc.SHAPES["D"]["synth"], aread_range=(996, 1004)))
        ovl, sel = pyoracle.pile_select(d.ovl, d.piles)
        kw = wc.params("WD")
    else:
        d, ovl, sel = wc.shape(name)
        kw = wc.params(name)
    E = engine.Engine(default_params(**kw)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fr, ba = E(sel, ovl, d.trace)
    t = E.timing_wide()
    first = dict(window_ms=round(t.window_ms, 2), last_ms=round(t.last_ms, 2), wdeep_ms=round(t.wdeep_ms, 2), total_ms=round(t.total_ms, 2))
    win, lms, wms = [], [], []
    for _ in range(steps):
        E.rerun(); fr, ba = E.collect(); t = E.timing_wide()
        win.append(round(t.window_ms, 2)); lms.append(round(t.last_ms, 2)); wms.append(round(t.wdeep_ms, 2))
    wx = E.debug_windows()
    print(json.dumps({"lib": os.path.basename(os.environ.get("DACC_LIB", "libdaccord_hip.so")), "shape": name, "params": kw, "piles": len(sel), "nwindows": int(t.nwindows),
                      "strings": [int(wx["mao"].min()), int(wx["mao"].max())], "deep": int((wx["mao"] > wc.MINS).sum()), "submit": first, "window_ms": win, "last_ms": lms, "wdeep_ms": wms,
                      "last": [int(t.last_windows), int(t.last_out)], "wdeep": [int(t.wdeep_windows), int(t.wdeep_out)], "tier_out": [int(x) for x in t.tier_out],
                      "long_windows": int(t.long_windows), "bases": len(ba), "sha": hashlib.sha256(engine.fasta(fr, ba).encode()).hexdigest()[:16]}), flush=True)
    E.close()


main()

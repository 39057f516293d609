"""The long string stage (k_window_fast<17>) against a library without it, one process per library (DACC_LIB selects it; a process cannot change
libraries): config 2's data set (scripts/sweep_env.py) at a wide window, one submit and `steps` resident passes, one JSON line with the times of
every pass and the second stream's counters.  A library whose dacc_timing ends at 176 bytes leaves the long string fields zero.
usage: [DACC_LIB=<lib.so>] python scripts/longstr_measure.py <reads> <w> <a> [steps=3] [k=14]"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from daccord_amd import engine
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData


def main():
    reads, w, a = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    steps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    k = int(sys.argv[5]) if len(sys.argv) > 5 else 14
    d = SynthData(int(reads * 10000 / 20), reads, 10000, seed=3, nthreads=min(16, os.cpu_count() or 1))
    ovl, piles = engine.pile_select(d.ovl, d.piles)
    E = engine.Engine(default_params(k=k, w=w, a=a)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fr, ba = E(piles, ovl, d.trace)
    t = E.timing_long()
    first = dict(window_ms=round(t.window_ms, 2), total_ms=round(t.total_ms, 2))
    win, tot, lms = [], [], []
    for _ in range(steps):
        E.rerun(); fr, ba = E.collect(); t = E.timing_long()
        win.append(round(t.window_ms, 2)); tot.append(round(t.total_ms, 2)); lms.append(round(t.longstr_ms, 2))
    h = hashlib.sha256(); well = 0
    for i in range(0, len(fr), 256):
        h.update(engine.fasta(fr[i:i + 256], ba, start_well=well).encode()); well += len(fr[i:i + 256])
    print(json.dumps({"lib": os.path.basename(os.environ.get("DACC_LIB", "libdaccord_hip.so")), "reads": reads, "k": k, "w": w, "a": a, "nwindows": int(t.nwindows), "submit": first,
                      "window_ms": win, "total_ms": tot, "long_windows": int(t.long_windows), "longstr_windows": int(t.longstr_windows), "longstr_out": int(t.longstr_out),
                      "longstr_ms": lms, "tier_out": [int(x) for x in t.tier_out], "last_windows": int(t.last_windows), "last_out": int(t.last_out), "bases": len(ba),
                      "sha": h.hexdigest()[:16]}), flush=True)
    E.close()


main()

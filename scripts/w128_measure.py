"""The stage of w = 128 (k_window_fast<20>) on the shapes of tests/w128_cases.py and on config 2's data set, one process per library and switch setting
(DACC_LIB selects the library, DACC_W128_TIER=0 the route from before the stage; a process cannot change libraries): one submit and `steps` passes of
dacc_rerun_resident, one JSON line with the times of every pass (device events of dacc_timing), the stage's counters and a digest of the FASTA.  A library whose
dacc_timing ends at 224 bytes leaves the w128 fields zero.
usage: [DACC_LIB=<lib.so>] [DACC_W128_TIER=0] python scripts/w128_measure.py <shape: A | D | E | S | K> [steps=3]
       [DACC_LIB=<lib.so>] [DACC_W128_TIER=0] python scripts/w128_measure.py cfg2 <reads> [steps=3] [k=14] [a=32]"""
import ctypes as C
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from daccord_amd import engine
from daccord_amd._structs import default_params, DaccTimingW128
from daccord_amd.synth import SynthData


def timing(E):
    """the 240 byte record; a library that knows fewer bytes fills what it knows and the rest stays zero"""
    t = DaccTimingW128()
    E._chk(E.L.dacc_last_timing2(E.h, C.byref(t), C.sizeof(DaccTimingW128)))
    return t


def main():
    name = sys.argv[1]
    if name == "cfg2":
        reads = int(sys.argv[2]); steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
        k = int(sys.argv[4]) if len(sys.argv) > 4 else 14; a = int(sys.argv[5]) if len(sys.argv) > 5 else 32
        d = SynthData(int(reads * 10000 / 20), reads, 10000, seed=3, nthreads=min(16, os.cpu_count() or 1))
        ovl, sel = engine.pile_select(d.ovl, d.piles)
        par = default_params(k=k, w=128, a=a); tr, tb = d.trace, d.trace_bytes
        what = dict(shape="cfg2", reads=reads, k=k, a=a)
    else:
        import w128_cases as WC
        steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
        d, ovl, sel, tr, tb = WC.shape(name)
        par = WC.params(name); what = dict(shape=name, **WC.SHAPES[name]["par"])
    E = engine.Engine(par); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fr, ba = E(sel, ovl, tr, trace_bytes=tb)
    t = timing(E)
    first = dict(window_ms=round(t.window_ms, 2), w128_ms=round(t.w128_ms, 2), total_ms=round(t.total_ms, 2))
    win, sms = [], []
    for _ in range(steps):
        E.rerun(); fr, ba = E.collect(); t = timing(E)
        win.append(round(t.window_ms, 2)); sms.append(round(t.w128_ms, 2))
    h = hashlib.sha256(); well = 0
    for i in range(0, len(fr), 256):
        h.update(engine.fasta(fr[i:i + 256], ba, start_well=well).encode()); well += len(fr[i:i + 256])
    print(json.dumps(dict(what, lib=os.path.basename(os.environ.get("DACC_LIB", "libdaccord_hip.so")), stage=os.environ.get("DACC_W128_TIER", "1") != "0", piles=len(sel),
                          nwindows=int(t.nwindows), submit=first, window_ms=win, w128_ms=sms, w128=[int(t.w128_windows), int(t.w128_out)],
                          tier_out=[int(x) for x in t.tier_out], long_windows=int(t.long_windows), bases=len(ba), sha=h.hexdigest()[:16])), flush=True)
    E.close()


main()

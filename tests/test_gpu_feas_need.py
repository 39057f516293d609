"""The filter of computeStretchFeasLanes on the device (only the (stretch, direction, start position) triples the enumerations can read get a
task): the cases of tests/feas_need_cases.py through the real kernels, with the filter and with DACC_FEAS_NEED=0 (read in dacc_create) --
per-window records, fragments, bases and FASTA of both runs equal the live oracle, hence each other, no pile dropped and no message.  One
case of tests/lowcomplex_cases.py is also held to the oracle digests committed in tests/golden/lowcomplex.json, with either setting.
That nothing the filter leaves out is ever read is asserted on the emulation (tests/test_feas_need.py).  Run with -m gpu."""
import json
import os

import pytest
import pyoracle
import feas_need_cases as fn
import lowcomplex_cases as lc
from daccord_amd import engine
from common import sha, windows_equal, frags_equal

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lowcomplex.json")


def _run(params, d, ovl, sel):
    E = engine.Engine(params); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(sel, ovl, d.trace, trace_bytes=getattr(d, "trace_bytes", 1))
    t = E.timing()
    wx = E.debug_windows()
    st, msgs = E.pile_status()
    assert len(st) == len(sel) and not st.any() and msgs == [], (st, msgs)
    E.close()
    return wx, fx, bx, t


@pytest.mark.parametrize("name", sorted(fn.CASES))
def test_device_with_and_without_the_filter(name, monkeypatch):
    wo, fo, bo = fn.oracle(name)
    d, ovl, sel = fn.shape(name)
    for need in ("1", "0"):
        monkeypatch.setenv("DACC_FEAS_NEED", need)
        wx, fx, bx, t = _run(fn.params(name), d, ovl, sel)
        print("feas need %s (DACC_FEAS_NEED=%s): windows %d, first_tier %d, tier_out %s, tier0 in / out %d / %d, tier7 in / out %d / %d, last_windows %d, window_ms %.2f" %
              (name, need, len(wo), t.first_tier, list(t.tier_out), t.tier0_in, t.tier0_out, t.tier7_in, t.tier7_out, t.last_windows, t.window_ms))
        bad = windows_equal(wo, wx)
        assert bad == [], (need, len(bad), bad[:5])
        assert frags_equal(fo, bo, fx, bx) and bytes(bx) == bytes(bo) and engine.fasta(fx, bx) == pyoracle.fasta(fo, bo)
        # the window kernels ran: the tiers, not the generic engine alone
        assert t.tier_ms[0] > 0 or t.tier_ms[1] > 0


def _digests(w, fr, ba, fasta):
    rows = []
    for x in w:
        r = [int(x["pile"]), int(x["y"]), int(x["status"]), int(x["mao"]), int(x["elength"])]
        if x["status"] == 1:
            r += [int(x["conslen"]), bytes(x["cons"]).hex(), int(x["minrate"]), int(x["filterfreq"]), int(x["k"])]
        rows.append(r)
    frows = [[int(y["aread"]), int(y["first"]), int(y["last"]), int(y["len"])] for y in fr]
    return {"windows": [len(rows), sha(json.dumps(rows))], "frags": [len(fr), sha(json.dumps(frows))], "bases": [len(ba), sha(bytes(ba))], "fasta": sha(fasta)}


@pytest.mark.parametrize("need", ["1", "0"])
def test_committed_digests(need, monkeypatch):
    """tests/golden/lowcomplex.json (the oracle's digests, as tests/test_lowcomplex.py computes them) for k14_mixed: cyclic graphs at the benchmark's k"""
    name = "k14_mixed"
    gold = json.load(open(GOLD))["cases"][name]
    monkeypatch.setenv("DACC_FEAS_NEED", need)
    d, ovl, sel = lc.shape(name)
    wx, fx, bx, t = _run(lc.params(name), d, ovl, sel)
    assert t.first_tier == 1 and t.tier_ms[0] > 0
    assert _digests(wx, fx, bx, engine.fasta(fx, bx)) == gold

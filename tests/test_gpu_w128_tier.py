"""The stage of w = 128 (k_window_fast<20>: every window of a batch with -w 128, layout in device memory, in front of k_window) on the device, through the
C ABI and with default switches: per-window records, fragments, bases and FASTA equal the live oracle, on the first pass, after a resident rerun and for a
second batch on the same context; the counters of dacc_last_timing2 add up to the windows of the batch; no slot, no trailing stage and no second stream run.
Shapes: tests/w128_cases.py.  Run with -m gpu."""
import ctypes as C
import numpy as np
import pytest
import pyoracle
import w128_cases as WC
from daccord_amd import engine
from daccord_amd._structs import default_params, DaccTimingWide, DaccTimingW128
from daccord_amd.synth import SynthData
from common import windows_equal, frags_equal

pytestmark = pytest.mark.gpu


def _engine(name):
    d = WC.shape(name)[0]
    E = engine.Engine(WC.params(name)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    return E


def _device_run(name):
    d, ovl, sel, tr, tb = WC.shape(name)
    E = _engine(name)
    fx, bx = E(sel, ovl, tr, trace_bytes=tb)
    return E, fx, bx


def _report(what, t):
    print("w128 %s: windows %d, w128_ms %.2f, w128_windows %d, w128_out %d, window_ms %.2f, tier_ms %s, tier_out %s, last_ms %.2f, long_windows %d"
          % (what, t.nwindows, t.w128_ms, t.w128_windows, t.w128_out, t.window_ms, list(t.tier_ms), list(t.tier_out), t.last_ms, t.long_windows))


def _same(E, ref, fx, bx):
    wo, fo, bo = ref
    st, msgs = E.pile_status()
    return (windows_equal(wo, E.debug_windows()) == [] and frags_equal(fo, bo, fx, bx) and pyoracle.fasta(fx, bx) == pyoracle.fasta(fo, bo)
            and not st.any() and msgs == [])


def _stage_alone(t, nwin):
    """the stage ran over every window of the batch and nothing else of the chain did"""
    assert t.nwindows == nwin
    assert t.w128_ms > 0 and t.w128_windows + t.w128_out == nwin and t.pad5_ == 0
    assert 20 * t.w128_out <= nwin
    assert list(t.tier_ms) == [0.0, 0.0, 0.0] and list(t.tier_out) == [0, 0, 0] and t.last_ms == 0.0 and t.long_windows == 0
    assert t.window_ms >= t.w128_ms


@pytest.mark.parametrize("name", ["A", "D", "E", "S"])
def test_w128_batches_equal_the_oracle_and_finish_in_the_stage(name):
    ref = WC.oracle(name); WC.check(name, ref[0])
    E, fx, bx = _device_run(name)
    t = E.timing_w128(); _report(name, t)
    assert _same(E, ref, fx, bx)
    _stage_alone(t, len(ref[0]))
    if name == "S":
        assert 1 <= t.w128_out <= 3      # the window with the string of 256 bases, and its half-overlapping neighbours that have one too
    # the resident batch again
    E.rerun(); f2, b2 = E.collect(); t2 = E.timing_w128()
    assert _same(E, ref, f2, b2)
    assert (t2.w128_windows, t2.w128_out) == (t.w128_windows, t.w128_out)
    _stage_alone(t2, len(ref[0]))
    # other piles on the same context
    d, ovl, sel, tr, tb = WC.shape(name)
    sel2 = WC.other_piles(name, 1)
    ref2 = WC.oracle_of(name, sel2)
    f3, b3 = E(sel2, ovl, tr, trace_bytes=tb); t3 = E.timing_w128(); _report(name + ", second batch", t3)
    assert _same(E, ref2, f3, b3)
    _stage_alone(t3, len(ref2[0]))
    E.close()


def test_a_w40_batch_on_a_second_context_does_not_launch_the_stage():
    E, fx, bx = _device_run("A")
    t = E.timing_w128()
    assert t.w128_ms > 0
    d, ovl, sel, tr, tb = WC.shape("A")
    p = default_params(k=12)
    O = pyoracle.Oracle(p); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
    fo, bo = O.run(sel[:1], ovl, tr, trace_bytes=tb, nthreads=8, want_windows=True)
    E2 = engine.Engine(p); E2.set_error_profile(*d.error_profile()); E2.load_db(d.bps, d.boff, d.rlen)
    f2, b2 = E2(sel[:1], ovl, tr, trace_bytes=tb)
    t2 = E2.timing_w128(); _report("A's first pile at w = 40", t2)
    assert windows_equal(O.windows(), E2.debug_windows()) == [] and frags_equal(fo, bo, f2, b2)
    assert t2.w128_ms == 0.0 and (t2.w128_windows, t2.w128_out, t2.pad5_) == (0, 0, 0)
    assert t2.tier_ms[0] > 0
    # the first context still has its stage
    E.rerun(); t1 = E.timing_w128()
    assert t1.w128_ms > 0 and t1.w128_windows == t.w128_windows
    E.close(); E2.close()


def test_switched_off_every_window_runs_in_the_generic_engine(monkeypatch):
    """DACC_W128_TIER=0 on shape A: the route from before the stage, the same output"""
    ref = WC.oracle("A"); WC.check("A", ref[0])
    E, fx, bx = _device_run("A")
    t = E.timing_w128(); E.close()
    monkeypatch.setenv("DACC_W128_TIER", "0")
    E0, f0, b0 = _device_run("A")
    t0 = E0.timing_w128(); _report("A, DACC_W128_TIER=0", t0)
    print("w128 A: window_ms %.2f with the stage, %.2f with DACC_W128_TIER=0" % (t.window_ms, t0.window_ms))
    assert _same(E0, ref, f0, b0) and frags_equal(fx, bx, f0, b0)
    assert t0.w128_ms == 0.0 and (t0.w128_windows, t0.w128_out) == (0, 0)
    assert list(t0.tier_ms) == [0.0, 0.0, 0.0] and list(t0.tier_out) == [0, 0, 0] and t0.last_ms == 0.0 and t0.long_windows == 0 and t0.window_ms > 0
    E0.close()


def test_record_grows_by_16_bytes_and_the_earlier_seam_holds():
    assert (C.sizeof(DaccTimingWide), C.sizeof(DaccTimingW128)) == (224, 240)
    E, fx, bx = _device_run("S")
    tw = E.timing_wide(); t = E.timing_w128()
    assert t.w128_windows > 0 and t.w128_ms > 0
    assert bytes(t)[:224] == bytes(tw)
    for size in (224, 232):
        buf = DaccTimingW128(); C.memset(C.byref(buf), 0xEE, C.sizeof(buf))
        assert E.L.dacc_last_timing2(E.h, C.byref(buf), size) == 0
        assert bytes(buf)[:224] == bytes(tw) and bytes(buf)[224:] == b"\xee" * 16, size
    big = (C.c_uint8 * 256)(); C.memset(big, 0xEE, 256)
    assert E.L.dacc_last_timing2(E.h, big, 240) == 0
    assert bytes(big)[:240] == bytes(t) and bytes(big)[240:] == b"\xee" * 16 and t.pad5_ == 0
    E.close()

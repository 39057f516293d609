"""The deepest stage (k_window_fast<16>: windows of 1001 ... 2000 strings and what tier 15 overflowed on, layout in device memory, behind the very
deep stage and in front of k_window) on the device, through the C ABI: per-window records and fragments equal the live oracle, the counters of
dacc_last_timing2 add up to the oracle's window depths, and the stage is not launched where no window needs it.  Shapes: tests/xdeep_cases.py.
No case sends a window of more than 1000 strings into k_window: its time there has never been measured.  Run with -m gpu."""
import ctypes as C
import pytest
import pyoracle
import xdeep_cases as xc
from daccord_amd import engine
from daccord_amd._structs import default_params, DaccTiming
from daccord_amd.synth import SynthData
from common import windows_equal, frags_equal

pytestmark = pytest.mark.gpu
SIZE_BEFORE = 160      # sizeof(dacc_timing) before the very deep stage's fields were appended


def _device_run(name, **kw):
    d, ovl, sel = xc.shape(name)
    E = engine.Engine(default_params(**kw)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(sel, ovl, d.trace)
    return E, fx, bx


def _report(what, t, n):
    print("xdeep %s: windows %d, xdeep_windows %d, xdeep_out %d, xdeep_ms %.2f, vdeep_windows %d, vdeep_out %d, vdeep_ms %.2f, last_ms %.2f, last_windows %d, last_out %d, tier_out %s, window_ms %.2f" %
          (what, n, t.xdeep_windows, t.xdeep_out, t.xdeep_ms, t.vdeep_windows, t.vdeep_out, t.vdeep_ms, t.last_ms, t.last_windows, t.last_out, list(t.tier_out), t.window_ms))


@pytest.mark.parametrize("k", [14, 8])
def test_pile_of_up_to_1932_strings_finishes_in_the_two_stages(k):
    """k = 8: the CPU emulation of the same code hands on nothing there (tests/test_xdeep_tier.py), so nothing reaches k_window"""
    wo, fo, bo = xc.oracle("P", k=k); xc.check("P", wo)
    E, fx, bx = _device_run("P", k=k)
    wx = E.debug_windows(); t = E.timing()
    _report("P k=%d" % k, t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.xdeep_out == 0 and t.xdeep_ms > 0 and t.xdeep_windows >= 28
    assert t.vdeep_windows + t.xdeep_windows == 37
    assert t.vdeep_out == t.xdeep_windows + t.xdeep_out      # what the very deep stage handed on is what this one read
    E.rerun(); f2, b2 = E.collect(); t2 = E.timing()
    assert frags_equal(fo, bo, f2, b2)
    assert (t2.xdeep_windows, t2.xdeep_out, t2.vdeep_windows, t2.vdeep_out, t2.last_windows, t2.last_out, list(t2.tier_out)) == \
           (t.xdeep_windows, t.xdeep_out, t.vdeep_windows, t.vdeep_out, t.last_windows, t.last_out, list(t.tier_out))
    E.close()


@pytest.mark.parametrize("maxalign", [1001, 2000])
def test_exactly_1001_and_2000_strings_finish_in_the_stage(maxalign):
    wo, fo, bo = xc.oracle("Q", maxalign=maxalign); xc.check("Q", wo, maxalign)
    E, fx, bx = _device_run("Q", k=14, maxalign=maxalign)
    wx = E.debug_windows(); t = E.timing()
    _report("Q -d %d" % maxalign, t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.xdeep_windows == 37 and t.xdeep_out == 0
    E.close()


def test_without_the_stages_in_front_it_reads_the_last_slots_list(monkeypatch):
    """DACC_LAST_TIER=0 and DACC_VDEEP_TIER=0: no trailing stage in front of it, so the stage takes what the third slot handed on.  The 37 windows of exactly
    1001 strings are those tiers 13 and 15 refuse at their string count in the default run: tier 16 sees no window it does not see there, and none of more
    than 1000 strings reaches k_window"""
    monkeypatch.setenv("DACC_LAST_TIER", "0"); monkeypatch.setenv("DACC_VDEEP_TIER", "0")
    wo, fo, bo = xc.oracle("Q", maxalign=1001)
    E, fx, bx = _device_run("Q", k=14, maxalign=1001)
    wx = E.debug_windows(); t = E.timing()
    _report("Q -d 1001, no last and no very deep stage", t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.xdeep_windows == 37 and t.xdeep_out == 0
    assert t.last_ms == 0.0 and t.vdeep_ms == 0.0
    assert t.xdeep_ms > 0
    E.close()


def test_what_the_very_deep_stage_refused_at_1000_strings_finishes():
    wo, fo, bo = xc.oracle("X"); xc.check("X", wo)
    E, fx, bx = _device_run("X", k=14)
    wx = E.debug_windows(); t = E.timing()
    _report("X", t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.xdeep_windows == 30 and t.xdeep_out == 0
    E.close()


def test_shallow_batch_does_not_launch_the_stage():
    """the shape of __graft_entry__.smoke(): no window of more than 1000 strings, so no slab and no launch"""
    d = SynthData(60000, 150, 3000, seed=2)
    ovl, piles = engine.pile_select(d.ovl, d.piles)
    p = default_params(k=8)
    E = engine.Engine(p); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(piles[:6], ovl, d.trace)
    O = pyoracle.Oracle(p); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
    fo, bo = O.run(piles[:6], ovl, d.trace, nthreads=4)
    t = E.timing()
    assert frags_equal(fo, bo, fx, bx)
    assert t.xdeep_ms == 0.0 and (t.xdeep_windows, t.xdeep_out) == (0, 0)
    assert C.sizeof(DaccTiming) == 176
    full = DaccTiming(); C.memset(C.byref(full), 0xEE, C.sizeof(full))
    assert E.L.dacc_last_timing2(E.h, C.byref(full), SIZE_BEFORE) == 0
    assert bytes(full)[:SIZE_BEFORE] == bytes(t)[:SIZE_BEFORE] and bytes(full)[SIZE_BEFORE:] == b"\xee" * 16
    E.close()


def test_record_keeps_its_size_and_the_fields_sit_in_the_pad_words():
    E, fx, bx = _device_run("X", k=14)
    t = E.timing()
    assert C.sizeof(DaccTiming) == 176 and DaccTiming.vdeep_ms.offset == SIZE_BEFORE
    assert (DaccTiming.xdeep_out.offset, DaccTiming.xdeep_ms.offset, DaccTiming.xdeep_windows.offset) == (124, 140, 156)
    assert t.xdeep_windows == 30 and t.xdeep_ms > 0
    full = DaccTiming(); C.memset(C.byref(full), 0xEE, C.sizeof(full))
    assert E.L.dacc_last_timing2(E.h, C.byref(full), SIZE_BEFORE) == 0
    assert bytes(full)[:SIZE_BEFORE] == bytes(t)[:SIZE_BEFORE] and bytes(full)[SIZE_BEFORE:] == b"\xee" * 16
    E.close()

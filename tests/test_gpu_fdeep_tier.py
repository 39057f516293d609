"""The full-depth stage (k_window_fast<18>: windows of 2001 ... 5001 strings and what tier 16 overflowed on, layout in device memory, behind the
deepest stage and in front of k_window) on the device, through the C ABI: per-window records and fragments equal the live oracle, the counters of
dacc_last_timing2 add up to the oracle's window depths, and the stage is not launched where no window needs it.  Shapes: tests/fdeep_cases.py and
shape P of tests/xdeep_cases.py.

No case sends a window of more than 2000 strings into k_window: its time there has never been measured.  Only (shape, k) pairs of which the CPU emulation
of the same code hands on nothing are run (tests/test_fdeep_tier.py: R at k = 14 and k = 8, Q at k = 14), and no DACC_*_TIER=0 switch is set.

Shape R+ (a pile of 6397 overlaps, more than any front end submits) stays a CPU case: whether the planner, the trace kernel and the vote are sized by
the 5000 overlaps of -D was not read through for this file.  Run with -m gpu."""
import ctypes as C
import pytest
import fdeep_cases as fc
import xdeep_cases as xc
from daccord_amd import engine
from daccord_amd._structs import default_params, DaccTiming, DaccTimingLong, DaccTimingFull
from common import windows_equal, frags_equal

pytestmark = pytest.mark.gpu


def _device_run(cases, name, **kw):
    d, ovl, sel = cases.shape(name)
    E = engine.Engine(default_params(**kw)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(sel, ovl, d.trace)
    return E, fx, bx


def _counters(t):
    return (t.fdeep_windows, t.fdeep_out, t.xdeep_windows, t.xdeep_out, t.vdeep_windows, t.vdeep_out, t.last_windows, t.last_out, list(t.tier_out))


def _report(what, t, n):
    print("fdeep %s: windows %d, fdeep_windows %d, fdeep_out %d, fdeep_ms %.2f, xdeep_windows %d, xdeep_out %d, xdeep_ms %.2f, vdeep_windows %d, vdeep_out %d, vdeep_ms %.2f, "
          "last_ms %.2f, last_windows %d, last_out %d, tier_out %s, window_ms %.2f" %
          (what, n, t.fdeep_windows, t.fdeep_out, t.fdeep_ms, t.xdeep_windows, t.xdeep_out, t.xdeep_ms, t.vdeep_windows, t.vdeep_out, t.vdeep_ms,
           t.last_ms, t.last_windows, t.last_out, list(t.tier_out), t.window_ms))


@pytest.mark.parametrize("k", [14, 8])
def test_deepest_pile_of_a_default_run_finishes_in_the_two_stages(k):
    wo, fo, bo = fc.oracle("R", k=k); fc.check("R", wo)
    E, fx, bx = _device_run(fc, "R", k=k)
    wx = E.debug_windows(); t = E.timing_full()
    _report("R k=%d" % k, t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.fdeep_out == 0 and t.fdeep_ms > 0
    assert t.xdeep_windows + t.fdeep_windows == 37 and t.fdeep_windows >= 34
    assert t.xdeep_out == t.fdeep_windows + t.fdeep_out      # what the deepest stage handed on is what this one read
    E.rerun(); f2, b2 = E.collect(); t2 = E.timing_full()
    assert frags_equal(fo, bo, f2, b2)
    assert _counters(t2) == _counters(t)
    E.close()


def test_exactly_2001_strings_finish_in_the_stage():
    wo, fo, bo = fc.oracle("Q", maxalign=2001); fc.check("Q", wo, 2001)
    E, fx, bx = _device_run(fc, "Q", k=14, maxalign=2001)
    wx = E.debug_windows(); t = E.timing_full()
    _report("Q -d 2001", t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.fdeep_windows == 37 and t.fdeep_out == 0
    # tiers 13, 15 and 16 refuse every window at its string count
    assert (t.last_windows, t.last_out) == (0, 37) and (t.vdeep_windows, t.vdeep_out) == (0, 37) and (t.xdeep_windows, t.xdeep_out) == (0, 37)
    E.close()


def test_pile_of_2070_to_3363_strings_finishes_in_the_stage():
    wo, fo, bo = fc.oracle("Q"); fc.check("Q", wo)
    E, fx, bx = _device_run(fc, "Q", k=14)
    wx = E.debug_windows(); t = E.timing_full()
    _report("Q", t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.fdeep_windows == 37 and t.fdeep_out == 0
    E.close()


def test_pile_of_up_to_1932_strings_does_not_launch_the_stage():
    """shape P of tests/xdeep_cases.py: no window of more than 2000 strings, so no slab and no launch; the older counters are those of
    tests/test_gpu_xdeep_tier.py"""
    wo, fo, bo = xc.oracle("P"); xc.check("P", wo)
    E, fx, bx = _device_run(xc, "P", k=14)
    wx = E.debug_windows(); t = E.timing_full()
    _report("P", t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.fdeep_ms == 0.0 and (t.fdeep_windows, t.fdeep_out, t.pad3_) == (0, 0, 0)
    assert t.xdeep_out == 0 and t.xdeep_ms > 0 and t.xdeep_windows >= 28
    assert t.vdeep_windows + t.xdeep_windows == 37
    assert t.vdeep_out == t.xdeep_windows + t.xdeep_out
    E.close()


def test_record_grows_by_16_bytes_and_the_earlier_seams_hold():
    assert (C.sizeof(DaccTiming), C.sizeof(DaccTimingLong), C.sizeof(DaccTimingFull)) == (176, 192, 208)
    assert (DaccTimingFull.fdeep_ms.offset, DaccTimingFull.fdeep_windows.offset, DaccTimingFull.fdeep_out.offset) == (192, 196, 200)
    E, fx, bx = _device_run(fc, "Q", k=14, maxalign=2001)
    tl = E.timing_long(); tf = E.timing_full()
    assert tf.fdeep_windows == 37 and tf.fdeep_ms > 0
    assert bytes(tf)[:192] == bytes(tl)
    for size in (192, 200):
        buf = DaccTimingFull(); C.memset(C.byref(buf), 0xEE, C.sizeof(buf))
        assert E.L.dacc_last_timing2(E.h, C.byref(buf), size) == 0
        assert bytes(buf)[:192] == bytes(tl) and bytes(buf)[192:] == b"\xee" * 16, size
    buf = DaccTimingFull(); C.memset(C.byref(buf), 0xEE, C.sizeof(buf))
    assert E.L.dacc_last_timing2(E.h, C.byref(buf), 208) == 0
    assert bytes(buf) == bytes(tf) and buf.fdeep_windows == 37 and buf.pad3_ == 0
    # the seam of the long string stage is where it was: a size in [176, 192) copies 176 bytes
    buf = DaccTimingFull(); C.memset(C.byref(buf), 0xEE, C.sizeof(buf))
    assert E.L.dacc_last_timing2(E.h, C.byref(buf), 184) == 0
    assert bytes(buf)[:176] == bytes(tl)[:176] and bytes(buf)[176:] == b"\xee" * 32
    E.close()

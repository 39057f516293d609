"""The wide deep stage (k_window_fast<19>: windows of 251 ... 1000 strings of a wide batch, layout in device memory, behind the last stage and in front of
k_window) on the device, through the C ABI and with default switches: per-window records and fragments equal the live oracle, the counters of
dacc_last_timing2 add up to the oracle's window depths, and the stage is not launched where no window needs it.  Shapes: tests/wdeep_cases.py.

The stage reads what the last stage (tier 14) handed on, which leaves out the windows the second stream has (a B string of more than 128 bases): with
D = the windows of more than 250 strings that are not on the second stream's list, wdeep_windows + wdeep_out == D.  At w = 64 no string of a window has
more than 128 bases (long_windows == 0 is asserted); in WD and WM every window the second stream has is counted out through long_windows, see _own().
Run with -m gpu."""
import ctypes as C
import numpy as np
import pytest
import vdeep_cases as vc
import wdeep_cases as wc
from daccord_amd import engine
from daccord_amd._structs import default_params, DaccTimingFull, DaccTimingWide
from common import windows_equal, frags_equal

pytestmark = pytest.mark.gpu


def _device_run(name):
    d, ovl, sel = wc.shape(name)
    E = engine.Engine(default_params(**wc.params(name))); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(sel, ovl, d.trace)
    return E, fx, bx


def _counters(t):
    return (t.wdeep_windows, t.wdeep_out, t.last_windows, t.last_out, list(t.tier_out), t.long_windows, t.longstr_windows, t.longstr_out,
            t.vdeep_windows, t.vdeep_out, t.xdeep_windows, t.xdeep_out, t.fdeep_windows, t.fdeep_out)


def _report(what, t, n):
    print("wdeep %s: windows %d, wdeep_windows %d, wdeep_out %d, wdeep_ms %.2f, last_ms %.2f, last_windows %d, last_out %d, tier_out %s, long_windows %d, longstr_windows %d, "
          "longstr_out %d, window_ms %.2f" % (what, n, t.wdeep_windows, t.wdeep_out, t.wdeep_ms, t.last_ms, t.last_windows, t.last_out, list(t.tier_out), t.long_windows,
                                              t.longstr_windows, t.longstr_out, t.window_ms))


def _own(name, wo, t):
    """D: the windows of more than 250 strings that are not on the second stream's list.  In every shape but WM all windows have more than 250 strings, so
    each window the second stream has (long_windows) is one of them; WM has no window on that list."""
    if name == "WM" or wc.params(name)["w"] == 64:
        assert t.long_windows == 0
    assert name == "WM" or wc.ndeep(wo) == len(wo)
    return wc.ndeep(wo) - t.long_windows


def _no_deep_stage_of_the_narrow_batches(t):
    assert (t.vdeep_ms, t.xdeep_ms, t.fdeep_ms) == (0.0, 0.0, 0.0)
    assert (t.vdeep_windows, t.vdeep_out, t.xdeep_windows, t.xdeep_out, t.fdeep_windows, t.fdeep_out) == (0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("name,out", [("WD", 0), ("WM", 0), ("S251", 0), ("S1000", 0), ("S1001", 9)])
def test_deep_wide_windows_equal_the_oracle_and_finish_in_the_stage(name, out):
    wo, fo, bo = wc.oracle(name); wc.check(name, wo)
    E, fx, bx = _device_run(name)
    wx = E.debug_windows(); t = E.timing_wide()
    _report(name, t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    D = _own(name, wo, t)
    assert t.wdeep_ms > 0 and t.wdeep_windows + t.wdeep_out == D and t.pad4_ == 0
    if out is not None:
        assert t.wdeep_out == out
    # tier 14 refuses every window of more than 250 strings at its string count: what it handed on holds all of this stage's.  Where every window is that
    # deep, tiers 8, 9 and 14 finish none (the first slot has no tier in a wide batch): each hands on the D windows it read
    assert t.last_out >= D
    if wc.ndeep(wo) == len(wo):
        assert (t.last_windows, t.last_out, list(t.tier_out)) == (0, D, [0, D, D])
    _no_deep_stage_of_the_narrow_batches(t)
    E.rerun(); f2, b2 = E.collect(); t2 = E.timing_wide()
    assert frags_equal(fo, bo, f2, b2)
    assert _counters(t2) == _counters(t)
    E.close()


def test_more_than_1000_strings_are_refused_at_their_string_count(monkeypatch):
    """S1001: what the stage hands on are the 9 windows of 1001 strings, with the flags of FFAIL(3).  (DACC_DEBUG_RETRY lists what the last slot handed on,
    all 62 windows, with the flags their last tier left: those the stage finished carry none.)"""
    monkeypatch.setenv("DACC_DEBUG_RETRY", "1")
    wo, fo, bo = wc.oracle("S1001"); wc.check("S1001", wo)
    E, fx, bx = _device_run("S1001")
    wx = E.debug_windows(); t = E.timing_wide(); r = E.debug_retry()
    print("wdeep S1001 retry list: %d windows, flags %s" % (len(r), sorted(set(hex(int(v)) for v in r[:, 1]))))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.wdeep_out == 9 and len(r) == 62
    refused = sorted(int(v) for v in r[r[:, 1] == 0x3000000, 0])
    assert refused == [int(i) for i in np.nonzero(wo["mao"] > wc.MAXS)[0]]
    E.close()


def test_exactly_250_strings_do_not_launch_the_stage():
    wo, fo, bo = wc.oracle("S250"); wc.check("S250", wo)
    E, fx, bx = _device_run("S250")
    wx = E.debug_windows(); t = E.timing_wide()
    _report("S250", t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.wdeep_ms == 0.0 and (t.wdeep_windows, t.wdeep_out, t.pad4_) == (0, 0, 0)
    assert t.long_windows == 0 and t.last_windows == 62 and t.last_out == 0      # tier 14's side of the seam
    E.close()


def test_narrow_batch_does_not_launch_the_stage():
    """shape M of tests/vdeep_cases.py at the default window: the very deep stage's batch, not this one's"""
    wo, fo, bo = vc.oracle("M"); vc.check("M", wo)
    d, ovl, sel = vc.shape("M")
    E = engine.Engine(default_params(k=14)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(sel, ovl, d.trace)
    wx = E.debug_windows(); t = E.timing_wide()
    _report("M (narrow)", t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.wdeep_ms == 0.0 and (t.wdeep_windows, t.wdeep_out, t.pad4_) == (0, 0, 0)
    assert t.vdeep_windows == 131 and t.vdeep_ms > 0
    E.close()


def test_switched_off_the_windows_run_where_they_ran_before(monkeypatch):
    """DACC_WDEEP_TIER=0 on S251: the chain as it was before the stage, 62 windows of 251 strings in k_window; every older counter is what the default
    run reports beside its own"""
    wo, fo, bo = wc.oracle("S251"); wc.check("S251", wo)
    E, fx, bx = _device_run("S251")
    t = E.timing_wide(); E.close()
    monkeypatch.setenv("DACC_WDEEP_TIER", "0")
    E0, f0, b0 = _device_run("S251")
    w0 = E0.debug_windows(); t0 = E0.timing_wide()
    _report("S251, DACC_WDEEP_TIER=0", t0, len(w0))
    assert windows_equal(wo, w0) == [] and frags_equal(fo, bo, f0, b0)
    assert t0.wdeep_ms == 0.0 and (t0.wdeep_windows, t0.wdeep_out) == (0, 0)
    assert (t0.last_windows, t0.last_out) == (0, 62)
    assert _counters(t0)[2:] == _counters(t)[2:]
    _no_deep_stage_of_the_narrow_batches(t0)
    E0.close()


def test_record_grows_by_16_bytes_and_the_earlier_seam_holds():
    assert (C.sizeof(DaccTimingFull), C.sizeof(DaccTimingWide)) == (208, 224)
    E, fx, bx = _device_run("S251")
    tf = E.timing_full(); tw = E.timing_wide()
    assert tw.wdeep_windows == 62 and tw.wdeep_ms > 0
    assert bytes(tw)[:208] == bytes(tf)
    for size in (208, 216):
        buf = DaccTimingWide(); C.memset(C.byref(buf), 0xEE, C.sizeof(buf))
        assert E.L.dacc_last_timing2(E.h, C.byref(buf), size) == 0
        assert bytes(buf)[:208] == bytes(tf) and bytes(buf)[208:] == b"\xee" * 16, size
    buf = DaccTimingWide(); C.memset(C.byref(buf), 0xEE, C.sizeof(buf))
    assert E.L.dacc_last_timing2(E.h, C.byref(buf), 224) == 0
    assert bytes(buf) == bytes(tw) and buf.wdeep_windows == 62 and buf.pad4_ == 0
    E.close()

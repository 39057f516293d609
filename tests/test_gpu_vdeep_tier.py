"""The very deep stage (k_window_fast<15>: windows of 251 ... 1000 strings, layout in device memory, behind the last stage and in front of
k_window) on the device, through the C ABI: per-window records and fragments equal the live oracle, the counters of dacc_last_timing2 add up
to the oracle's window depths, and the stage is not launched where no window needs it.  Shapes: tests/vdeep_cases.py.  Run with -m gpu."""
import ctypes as C
import pytest
import pyoracle
import vdeep_cases as vc
from daccord_amd import engine
from daccord_amd._structs import default_params, DaccTiming
from daccord_amd.synth import SynthData
from common import windows_equal, frags_equal

pytestmark = pytest.mark.gpu
SIZE_BEFORE = 160      # sizeof(dacc_timing) before vdeep_ms, vdeep_windows, vdeep_out and a pad word were appended


def _device_run(name, k):
    d, ovl, sel = vc.shape(name)
    E = engine.Engine(default_params(k=k)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(sel, ovl, d.trace)
    return E, fx, bx


def _report(what, t, n):
    print("vdeep %s: windows %d, vdeep_windows %d, vdeep_out %d, vdeep_ms %.2f, last_ms %.2f, last_windows %d, last_out %d, deep_windows %d, deep_out %d, tier_out %s, window_ms %.2f" %
          (what, n, t.vdeep_windows, t.vdeep_out, t.vdeep_ms, t.last_ms, t.last_windows, t.last_out, t.deep_windows, t.deep_out, list(t.tier_out), t.window_ms))


@pytest.mark.parametrize("k", [14, 8])
def test_deep_pile_finishes_in_the_stage(k):
    wo, fo, bo = vc.oracle("D", k=k); vc.check("D", wo)
    E, fx, bx = _device_run("D", k)
    wx = E.debug_windows(); t = E.timing()
    _report("D k=%d" % k, t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.vdeep_windows + t.vdeep_out == int((wo["mao"] > vc.MINS).sum()) == 197
    assert t.vdeep_out == 0               # the CPU emulation of the same code finishes all of them in the tier (tests/test_vdeep_tier.py)
    assert t.vdeep_ms > 0
    assert t.last_out == t.tier_out[2]    # tier 13 finishes none of them
    E.rerun(); f2, b2 = E.collect(); t2 = E.timing()
    assert frags_equal(fo, bo, f2, b2)
    assert (t2.vdeep_windows, t2.vdeep_out, t2.last_windows, t2.last_out, list(t2.tier_out)) == (t.vdeep_windows, t.vdeep_out, t.last_windows, t.last_out, list(t.tier_out))
    E.close()


def test_mixed_pile_splits_between_the_deep_tier_and_the_stage():
    wo, fo, bo = vc.oracle("M"); vc.check("M", wo)
    E, fx, bx = _device_run("M", 14)
    wx = E.debug_windows(); t = E.timing()
    _report("M", t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.vdeep_windows == 131 and t.vdeep_out == 0
    assert t.deep_windows == 76 and t.deep_out == 131
    E.close()


def test_switch_off_sends_them_to_the_generic_engine(monkeypatch):
    monkeypatch.setenv("DACC_VDEEP_TIER", "0")
    wo, fo, bo = vc.oracle("M")
    E, fx, bx = _device_run("M", 14)
    wx = E.debug_windows(); t = E.timing()
    _report("M, stage off", t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert (t.vdeep_windows, t.vdeep_out, t.vdeep_ms) == (0, 0, 0.0)
    E.close()


def test_without_the_last_stage_it_reads_the_last_slots_list(monkeypatch):
    """DACC_LAST_TIER=0: no trailing stage in front of it, so the stage takes what the third slot handed on; the same 131 windows finish in it"""
    monkeypatch.setenv("DACC_LAST_TIER", "0")
    wo, fo, bo = vc.oracle("M")
    E, fx, bx = _device_run("M", 14)
    wx = E.debug_windows(); t = E.timing()
    _report("M, no last stage", t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.vdeep_windows == 131 and t.vdeep_out == 0
    assert t.last_ms == 0.0 and (t.last_windows, t.last_out) == (0, 0)
    assert t.vdeep_ms > 0
    E.close()


def test_shallow_batch_does_not_launch_the_stage():
    """the shape of __graft_entry__.smoke(): no window of more than 250 strings, so no slab and no launch"""
    d = SynthData(60000, 150, 3000, seed=2)
    ovl, piles = engine.pile_select(d.ovl, d.piles)
    p = default_params(k=8)
    E = engine.Engine(p); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(piles[:6], ovl, d.trace)
    O = pyoracle.Oracle(p); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
    fo, bo = O.run(piles[:6], ovl, d.trace, nthreads=4)
    t = E.timing()
    assert frags_equal(fo, bo, fx, bx)
    assert t.vdeep_ms == 0.0 and (t.vdeep_windows, t.vdeep_out) == (0, 0)
    E.close()


def test_tier_as_the_third_slot(monkeypatch):
    """DACC_VDEEP_AS_SLOT2=1: the tier runs through the ordinary slot launch, tier 12 still in front of it, and no very deep stage behind"""
    monkeypatch.setenv("DACC_VDEEP_AS_SLOT2", "1")
    wo, fo, bo = vc.oracle("M")
    E, fx, bx = _device_run("M", 14)
    wx = E.debug_windows(); t = E.timing()
    _report("M, as slot 2", t, len(wx))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert t.vdeep_ms == 0.0
    E.close()


def test_last_timing2_with_the_size_before_the_stage():
    """a caller compiled against the record as it was before the stage's fields were appended keeps what it wrote behind it"""
    E, fx, bx = _device_run("M", 14)
    t = E.timing()
    assert C.sizeof(DaccTiming) == SIZE_BEFORE + 16 and DaccTiming.vdeep_ms.offset == SIZE_BEFORE and t.vdeep_windows > 0
    full = DaccTiming(); C.memset(C.byref(full), 0xEE, C.sizeof(full))
    assert E.L.dacc_last_timing2(E.h, C.byref(full), SIZE_BEFORE) == 0
    assert bytes(full)[:SIZE_BEFORE] == bytes(t)[:SIZE_BEFORE] and bytes(full)[SIZE_BEFORE:] == b"\xee" * 16
    E.close()

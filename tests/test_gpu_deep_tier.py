"""The deep-window tier (k_window_fast<12>: windows of 97 ... 250 strings, one wavefront per CU) on the device, through the C ABI: per-window
records and fragments equal the live oracle, and the counters of dacc_last_timing2 add up to the oracle's window depths.  Run with -m gpu."""
import ctypes as C
import pytest
import pyoracle
from daccord_amd import engine
from daccord_amd._structs import default_params, DaccTiming, TIMING_SIZE_V1
from daccord_amd.synth import SynthData
from common import windows_equal, frags_equal

pytestmark = pytest.mark.gpu
MINS, MAXS = 96, 250      # FastTier<12>::mins / maxs

_SHAPES = {"150x": ((30000, 900, 5000), 450), "250x": ((20000, 1000, 5000), 500)}
_data = {}
_oracle = {}


def _shape(name):
    """one pile from the middle of a seeded deep data set (about 500 windows: one per CU)"""
    if name not in _data:
        args, mid = _SHAPES[name]
        d = SynthData(*args, seed=21)
        ovl, piles = pyoracle.pile_select(d.ovl, d.piles)
        _data[name] = (d, ovl, piles[mid:mid + 1])
    return _data[name]


def _oracle_run(name, k):
    if (name, k) not in _oracle:
        d, ovl, sel = _shape(name)
        O = pyoracle.Oracle(default_params(k=k)); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
        fo, bo = O.run(sel, ovl, d.trace, nthreads=8, want_windows=True)
        _oracle[(name, k)] = (O.windows(), fo, bo)
    return _oracle[(name, k)]


def _device_run(name, k):
    d, ovl, sel = _shape(name)
    E = engine.Engine(default_params(k=k)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(sel, ovl, d.trace)
    return E, fx, bx


@pytest.mark.parametrize("name,k", [("150x", 14), ("150x", 8), ("250x", 14)])
def test_deep_windows_equal_the_oracle_and_are_counted(name, k):
    wo, fo, bo = _oracle_run(name, k)
    E, fx, bx = _device_run(name, k)
    wx = E.debug_windows(); t = E.timing()
    print("deep tier %s k=%d: windows %d, deep_windows %d, deep_out %d, deep_ms %.2f, tier_ms %s, tier_out %s, window_ms %.2f" %
          (name, k, len(wx), t.deep_windows, t.deep_out, t.deep_ms, list(t.tier_ms), list(t.tier_out), t.window_ms))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    mao = wo["mao"]
    nin = int(((mao > MINS) & (mao <= MAXS)).sum()); nover = int((mao > MAXS).sum())
    assert nin > 0 and (nover > 0) == (name == "250x")
    assert t.deep_windows + t.deep_out == nin + nover                 # every window of more than 96 strings reaches the tier
    assert t.deep_out >= nover                                         # more than 250 strings: handed on
    assert t.deep_windows == nin - (t.deep_out - nover)
    # the CPU emulation of the same code finishes every window of 97 ... 250 strings of these shapes in the tier (tests/test_deep_tier.py)
    assert t.deep_windows == nin and t.deep_ms > 0
    assert t.tier_out[2] == t.deep_out                                 # tier 3 holds none of them: the generic engine runs what the tier handed on
    E.rerun(); f2, b2 = E.collect(); t2 = E.timing()
    assert frags_equal(fo, bo, f2, b2) and (t2.deep_windows, t2.deep_out) == (t.deep_windows, t.deep_out)
    E.close()


def test_switch_off_sends_deep_windows_to_the_generic_engine(monkeypatch):
    monkeypatch.setenv("DACC_DEEP_TIER", "0")
    wo, fo, bo = _oracle_run("150x", 14)
    E, fx, bx = _device_run("150x", 14)
    wx = E.debug_windows(); t = E.timing()
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    assert (t.deep_windows, t.deep_out, t.deep_ms) == (0, 0, 0.0)
    assert t.tier_out[2] == int((wo["mao"] > MINS).sum())
    E.close()


def test_last_timing_fills_only_the_first_version_of_the_record():
    """dacc_last_timing keeps the signature it had before the record grew: a caller with the earlier, shorter struct is not overrun.
    dacc_last_timing2 copies what the caller has room for."""
    E, fx, bx = _device_run("150x", 14)
    GUARD = 0xA5A5A5A55A5A5A5A

    class Guarded(C.Structure):
        _fields_ = [("old", C.c_uint8 * TIMING_SIZE_V1), ("guard", C.c_uint64)]
    g = Guarded(); g.guard = GUARD
    assert E.L.dacc_last_timing(E.h, C.cast(C.byref(g), C.POINTER(DaccTiming))) == 0
    assert g.guard == GUARD
    t = E.timing()
    assert bytes(g.old) == bytes(t)[:TIMING_SIZE_V1] and t.nwindows > 0 and t.deep_windows > 0
    # a size in the middle of the new part: the fields behind it stay as the caller set them
    full = DaccTiming(); C.memset(C.byref(full), 0xEE, C.sizeof(full))
    assert E.L.dacc_last_timing2(E.h, C.byref(full), TIMING_SIZE_V1 + 8) == 0
    assert bytes(full)[:TIMING_SIZE_V1 + 8] == bytes(t)[:TIMING_SIZE_V1 + 8] and bytes(full)[TIMING_SIZE_V1 + 8:] == b"\xee" * (C.sizeof(full) - TIMING_SIZE_V1 - 8)
    # a larger size than the library's record: no more than the record is written
    class Larger(C.Structure):
        _fields_ = [("t", DaccTiming), ("guard", C.c_uint64)]
    big = Larger(); big.guard = GUARD
    assert E.L.dacc_last_timing2(E.h, C.cast(C.byref(big), C.POINTER(DaccTiming)), C.sizeof(big)) == 0
    assert big.guard == GUARD and bytes(big.t) == bytes(t)
    E.close()

"""The last stage of the tier chain on the device, through the C ABI: k_window_fast<13> (wide batches: <14>), the tiers whose layout lives in a
slab of device memory, take what the last enabled slot handed on and hand on to the generic engine.  Per-window records and fragments equal
the live oracle on every route and the counters last_ms / last_windows / last_out of dacc_last_timing2 say where the windows finished.
Shapes: tests/last_tier_cases.py.  Run with -m gpu."""
import pytest
import last_tier_cases as LC
from daccord_amd import engine
from common import windows_equal, frags_equal

pytestmark = pytest.mark.gpu


def _device_run(name, monkeypatch, **env):
    for k in ("DACC_TIERS", "DACC_LAST_TIER", "DACC_LAST_AS_SLOT2"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(LC.SHAPES[name]["env"], **env).items():
        monkeypatch.setenv(k, v)
    d, ovl, sel = LC.shape(name)
    E = engine.Engine(LC.params(name)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(sel, ovl, d.trace)
    return E, fx, bx


def _check(name, E, fx, bx):
    wo, fo, bo = LC.oracle(name, nthreads=8)
    wx = E.debug_windows(); t = E.timing()
    print("last stage %s: windows %d, tier_out %s, last_windows %d, last_out %d, last_ms %.3f, tier_ms %s, window_ms %.2f" %
          (name, len(wx), list(t.tier_out), t.last_windows, t.last_out, t.last_ms, [round(x, 3) for x in t.tier_ms], t.window_ms))
    assert windows_equal(wo, wx) == [] and frags_equal(fo, bo, fx, bx)
    return t


@pytest.mark.parametrize("name,slot,least", [("A", 0, 100), ("W", 1, 20)])
def test_forced_route_finishes_in_the_last_stage(name, slot, least, monkeypatch):
    """what the only enabled slot hands on finishes in the stage: its capacities include those of every LDS tier, so a hand-over here is a defect"""
    E, fx, bx = _device_run(name, monkeypatch)
    t = _check(name, E, fx, bx)
    assert t.tier_out[slot] > least
    assert t.last_windows == t.tier_out[slot] and t.last_out == 0 and t.last_ms > 0
    fo, bo = LC.oracle(name)[1:]
    E.rerun(); f2, b2 = E.collect(); t2 = E.timing()
    assert frags_equal(fo, bo, f2, b2)
    assert (list(t2.tier_out), t2.last_windows, t2.last_out) == (list(t.tier_out), t.last_windows, t.last_out) and t2.last_ms > 0
    E.close()


def test_capacity_shape_default_chain(monkeypatch):
    """Shape H: the ten windows tier 3 hands on at its weight table finish in the stage, as in the emulation (tests/test_last_tier.py)"""
    E, fx, bx = _device_run("H", monkeypatch)
    t = _check("H", E, fx, bx)
    assert t.tier_out[2] == len(LC.H_WINDOWS) == 10
    assert t.last_windows + t.last_out == 10
    assert t.last_windows == LC.H_FINISHED and LC.H_FINISHED >= 8
    E.close()


def test_switch_off_restores_the_route_of_the_generic_engine(monkeypatch):
    E, fx, bx = _device_run("A", monkeypatch, DACC_LAST_TIER="0")
    t = _check("A", E, fx, bx)
    assert (t.last_windows, t.last_out, t.last_ms) == (0, 0, 0.0)
    assert t.tier_out[0] > 100
    E.close()


def test_tier_as_third_slot_equals_the_oracle(monkeypatch):
    E, fx, bx = _device_run("H", monkeypatch, DACC_LAST_AS_SLOT2="1")
    t = _check("H", E, fx, bx)
    assert (t.last_windows, t.last_out, t.last_ms) == (0, 0, 0.0)       # no last stage with the switch: the third slot is tier 13
    assert t.tier_out[2] == len(LC.H_WINDOWS) - LC.H_FINISHED
    E.close()

"""The very deep tier (FastTier<15>, daccord_amd/csrc/fast_window.hpp) on the CPU emulation: windows of 251 ... 1000 strings leave the generic
engine.  The emulation harness walks the slots of the chain only, so the tier is run as the third slot's main tier (DACC_VDEEP_AS_SLOT2=1, with
the deep-window tier 12 still in front of it); without the switch the harness counts what it counted before the stage existed.  Everything
equals the oracle bit for bit.

The resolved pipeline is not exposed to Python (dacc_plan_only returns window and block counts only), so that the stage is off in a batch
without a window of more than 250 strings, and with DACC_VDEEP_TIER=0, is asserted on the device through vdeep_ms == 0
(tests/test_gpu_vdeep_tier.py); here only the conflict of the two slot switches is checked, which dacc_create refuses before it looks for a device."""
import ctypes as C
import pytest
import pyoracle
import emul_lib
import vdeep_cases as vc
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData
from common import windows_equal, frags_equal


def _emul_run(data, lanes=1, **kw):
    d, ovl, sel = data
    E = emul_lib.Emul(default_params(**kw), lanes=lanes); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fe, be = E.run(sel, ovl, d.trace)
    return E, fe, be


def _front_count(E, nwindows):
    """windows that finished in the front tiers the harness keeps no counter for (the deep-window tier 12), as tests/test_deep_tier.py infers it"""
    return nwindows - (sum(E.counts()) + E.count_tier0() + E.count_tier7() + E.count_tier10() + E.count_long())


@pytest.mark.parametrize("lanes,k", [(1, 14), (64, 14), (1, 8)])
def test_deep_pile_finishes_in_the_tier(monkeypatch, lanes, k):
    monkeypatch.setenv("DACC_VDEEP_AS_SLOT2", "1")
    wo, fo, bo = vc.oracle("D", k=k); vc.check("D", wo)
    E, fe, be = _emul_run(vc.shape("D"), lanes=lanes, k=k)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    assert E.counts() == (0, 0, 197, 0), E.counts()


def test_mixed_pile_splits_at_250_strings(monkeypatch):
    monkeypatch.setenv("DACC_VDEEP_AS_SLOT2", "1")
    wo, fo, bo = vc.oracle("M"); vc.check("M", wo)
    E, fe, be = _emul_run(vc.shape("M"), k=14)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    assert E.counts() == (23, 5, 131, 0), E.counts()
    assert _front_count(E, len(wo)) == 76      # tier 12 still finishes the windows of 97 ... 250 strings


def test_more_than_1000_strings_are_handed_on(monkeypatch):
    monkeypatch.setenv("DACC_VDEEP_AS_SLOT2", "1")
    wo, fo, bo = vc.oracle("X"); vc.check("X", wo)
    E, fe, be = _emul_run(vc.shape("X"), k=14)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    assert E.counts()[2] == 167 and E.counts()[3] == 30, E.counts()


@pytest.mark.parametrize("name,counts", [("M", (23, 5, 0, 131)), ("D", (0, 0, 0, 197))])
def test_without_the_switch_the_harness_sees_no_new_stage(monkeypatch, name, counts):
    monkeypatch.delenv("DACC_VDEEP_AS_SLOT2", raising=False)
    wo, fo, bo = vc.oracle(name); vc.check(name, wo)
    E, fe, be = _emul_run(vc.shape(name), k=14)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    assert E.counts() == counts, E.counts()


def test_windows_of_at_most_250_strings_pass_through_untouched(monkeypatch):
    """The 50x pile of tests/test_deep_tier.py: as the third slot's main tier, tier 15 passes every window that reaches it on (none has more than
    250 strings) and the generic engine finishes those; what the tiers in front finish does not move."""
    d = SynthData(30000, 300, 5000, seed=7)
    ovl, piles = pyoracle.pile_select(d.ovl, d.piles)
    data = (d, ovl, piles[10:11])
    O = pyoracle.Oracle(default_params(k=14)); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
    fo, bo = O.run(data[2], ovl, d.trace, nthreads=4, want_windows=True)
    wo = O.windows()
    assert wo["mao"].max() <= vc.DEEP_MINS
    E0, f0, b0 = _emul_run(data, k=14)
    monkeypatch.setenv("DACC_VDEEP_AS_SLOT2", "1")
    E, fe, be = _emul_run(data, k=14)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    c0, c = E0.counts(), E.counts()
    assert c[:2] == c0[:2] and c[2] == 0 and c[3] == c0[2] + c0[3], (c0, c)
    assert (E.count_tier0(), E.count_tier7(), E.count_tier10()) == (E0.count_tier0(), E0.count_tier7(), E0.count_tier10())


def test_both_slot_switches_together_are_refused(monkeypatch):
    """DACC_LAST_AS_SLOT2=1 and DACC_VDEEP_AS_SLOT2=1 both name the third slot's main tier: dacc_create returns DACC_EINVAL (before it looks for a
    device, so this runs without one); either switch alone passes that check."""
    from daccord_amd import engine
    L = engine.lib()
    L.dacc_create.restype = C.c_int
    p = default_params(k=8)
    def create():
        h = C.c_void_p()
        rc = L.dacc_create(C.byref(h), C.byref(p))
        if rc == 0:
            L.dacc_destroy.argtypes = [C.c_void_p]; L.dacc_destroy(h)
        return rc
    EINVAL = -1
    monkeypatch.setenv("DACC_LAST_AS_SLOT2", "1"); monkeypatch.setenv("DACC_VDEEP_AS_SLOT2", "1")
    assert create() == EINVAL
    monkeypatch.delenv("DACC_LAST_AS_SLOT2")
    assert create() != EINVAL

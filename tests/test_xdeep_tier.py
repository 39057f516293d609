"""The deepest tier (FastTier<16>, daccord_amd/csrc/fast_window.hpp) on the CPU emulation: windows of 1001 ... 2000 strings leave the generic
engine.  The emulation harness walks the slots of the chain only, so the tier is run as the third slot's main tier (DACC_XDEEP_AS_SLOT2=1, with
the deep-window tier 12 still in front of it); without the switch the harness counts what it counted before the stage existed.  Everything
equals the oracle bit for bit.  Shapes: tests/xdeep_cases.py.

That the stage is off in a batch without a window of more than 1000 strings is asserted on the device through xdeep_ms == 0
(tests/test_gpu_xdeep_tier.py); here the conflict of the three slot switches is checked, which dacc_create refuses before it looks for a device.

The case of 2001 strings runs 37 windows through the emulated generic engine (measured: 1.7 s for the emulation of the case on one host lane, 2.3 s for the oracle); it is the only
check of the tier's upper seam."""
import ctypes as C
import itertools
import pytest
import emul_lib
import xdeep_cases as xc
from daccord_amd._structs import default_params
from common import windows_equal, frags_equal

# windows of shape P the tier hands on at k = 8 (emulation): none
P_K8_HANDED_ON = 0


def _emul_run(data, lanes=1, **kw):
    d, ovl, sel = data
    E = emul_lib.Emul(default_params(**kw), lanes=lanes); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fe, be = E.run(sel, ovl, d.trace)
    return E, fe, be


@pytest.mark.parametrize("lanes,k", [(1, 14), (64, 14), (1, 8)])
def test_pile_of_up_to_1932_strings_finishes_in_the_tier(monkeypatch, lanes, k):
    monkeypatch.setenv("DACC_XDEEP_AS_SLOT2", "1")
    wo, fo, bo = xc.oracle("P", k=k); xc.check("P", wo)
    E, fe, be = _emul_run(xc.shape("P"), lanes=lanes, k=k)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    if k == 14:
        assert E.counts() == (0, 0, 37, 0), E.counts()
    else:
        assert E.counts() == (0, 0, 37 - P_K8_HANDED_ON, P_K8_HANDED_ON), E.counts()


@pytest.mark.parametrize("maxalign", [1001, 2000])
def test_exactly_1001_and_2000_strings_finish_in_the_tier(monkeypatch, maxalign):
    monkeypatch.setenv("DACC_XDEEP_AS_SLOT2", "1")
    wo, fo, bo = xc.oracle("Q", maxalign=maxalign); xc.check("Q", wo, maxalign)
    E, fe, be = _emul_run(xc.shape("Q"), k=14, maxalign=maxalign)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    assert E.counts() == (0, 0, 37, 0), E.counts()


def test_2001_strings_are_handed_on(monkeypatch):
    monkeypatch.setenv("DACC_XDEEP_AS_SLOT2", "1")
    wo, fo, bo = xc.oracle("Q", maxalign=2001); xc.check("Q", wo, 2001)
    E, fe, be = _emul_run(xc.shape("Q"), k=14, maxalign=2001)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    assert E.counts() == (0, 0, 0, 37), E.counts()


def test_what_tier_15_refused_at_1000_strings_finishes(monkeypatch):
    monkeypatch.setenv("DACC_XDEEP_AS_SLOT2", "1")
    wo, fo, bo = xc.oracle("X"); xc.check("X", wo)
    E, fe, be = _emul_run(xc.shape("X"), k=14)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    assert E.counts()[2] == 197 and E.counts()[3] == 0, E.counts()


def test_without_the_switch_the_harness_sees_no_new_stage(monkeypatch):
    for name in ("DACC_XDEEP_AS_SLOT2", "DACC_VDEEP_AS_SLOT2", "DACC_LAST_AS_SLOT2"):
        monkeypatch.delenv(name, raising=False)
    wo, fo, bo = xc.oracle("P"); xc.check("P", wo)
    E, fe, be = _emul_run(xc.shape("P"), k=14)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    assert E.counts() == (0, 0, 0, 37), E.counts()


def test_more_than_one_slot_switch_is_refused(monkeypatch):
    """DACC_LAST_AS_SLOT2=1, DACC_VDEEP_AS_SLOT2=1 and DACC_XDEEP_AS_SLOT2=1 each name the third slot's main tier: with any two of them dacc_create
    returns DACC_EINVAL (before it looks for a device, so this runs without one); each alone passes that check."""
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
    names = ("DACC_LAST_AS_SLOT2", "DACC_VDEEP_AS_SLOT2", "DACC_XDEEP_AS_SLOT2")
    for n in names:
        monkeypatch.delenv(n, raising=False)
    for n in names:
        monkeypatch.setenv(n, "1")
        assert create() != EINVAL, n
        monkeypatch.delenv(n)
    for a, b in itertools.combinations(names, 2):
        monkeypatch.setenv(a, "1"); monkeypatch.setenv(b, "1")
        assert create() == EINVAL, (a, b)
        monkeypatch.delenv(a); monkeypatch.delenv(b)
    for n in names:
        monkeypatch.setenv(n, "1")
    assert create() == EINVAL

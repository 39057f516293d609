"""The full-depth tier (FastTier<18>, daccord_amd/csrc/fast_window.hpp) on the CPU emulation: windows of 2001 ... 5001 strings leave the generic
engine.  The emulation harness walks the slots of the chain only, so the tier is run as the third slot's main tier (DACC_FDEEP_AS_SLOT2=1, with
the deep-window tier 12 still in front of it); without the switch the harness counts what it counted before the stage existed.  Everything
equals the oracle bit for bit.  Shapes: tests/fdeep_cases.py.

That the stage is off in a batch without a window of more than 2000 strings is asserted on the device through fdeep_ms == 0
(tests/test_gpu_fdeep_tier.py); here the conflict of the four slot switches is checked, which dacc_create refuses before it looks for a device.

The case of 5002 strings runs 20 windows through the emulated generic engine; it is the only check of the tier's upper seam, on the CPU only.

Wall time of the file, measured on an 8 core host without a GPU: 61 s -- 35 s of it in the first case, which generates shape Q and runs the first
oracle; every other case takes 2 ... 5 s, the one on 64 emulated lanes 5 s, so both lane counts stay."""
import ctypes as C
import pytest
import emul_lib
import fdeep_cases as fc
from daccord_amd._structs import default_params
from common import windows_equal, frags_equal

# windows the tier hands on at k = 8 (emulation).  Shape R: none.  Shape Q: one window (6786 nodes in 5144 stretches), whose reverse enumerations
# together keep more paths than the pool of 4096 (rccap: 256 chunks of 16, the most an 8 bit chunk id names) -- the pool is tier 13's in every
# device-memory tier.  Shape Q at k = 8 is therefore no case of the device tests.
R_K8_HANDED_ON = 0
Q_K8_HANDED_ON = 1


def _emul_run(data, lanes=1, **kw):
    d, ovl, sel = data
    E = emul_lib.Emul(default_params(**kw), lanes=lanes); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fe, be = E.run(sel, ovl, d.trace)
    return E, fe, be


def _case(monkeypatch, name, k, maxalign, lanes, handed_on):
    monkeypatch.setenv("DACC_FDEEP_AS_SLOT2", "1")
    wo, fo, bo = fc.oracle(name, k=k, maxalign=maxalign); fc.check(name, wo, maxalign)
    kw = dict(k=k) if maxalign is None else dict(k=k, maxalign=maxalign)
    E, fe, be = _emul_run(fc.shape(name), lanes=lanes, **kw)
    print("fdeep emulation %s k=%d -d %s lanes %d: counts %s" % (name, k, maxalign, lanes, E.counts()))
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    assert E.counts() == (0, 0, 37 - handed_on, handed_on), E.counts()


@pytest.mark.parametrize("k,handed_on", [(14, 0), (8, Q_K8_HANDED_ON)])
def test_pile_of_2070_to_3363_strings_finishes_in_the_tier(monkeypatch, k, handed_on):
    _case(monkeypatch, "Q", k, None, 1, handed_on)


@pytest.mark.parametrize("lanes", [1, 64])
def test_exactly_2001_strings_finish_in_the_tier(monkeypatch, lanes):
    _case(monkeypatch, "Q", 14, 2001, lanes, 0)


@pytest.mark.parametrize("k,handed_on", [(14, 0), (8, R_K8_HANDED_ON)])
def test_deepest_pile_of_a_default_run_finishes_in_the_tier(monkeypatch, k, handed_on):
    _case(monkeypatch, "R", k, None, 1, handed_on)


def test_exactly_5001_strings_finish_in_the_tier(monkeypatch):
    _case(monkeypatch, "R+", 14, 5001, 1, 0)


def test_5002_strings_are_handed_on(monkeypatch):
    _case(monkeypatch, "R+", 14, 5002, 1, 20)


def test_without_the_switch_the_harness_sees_no_new_stage(monkeypatch):
    for name in ("DACC_FDEEP_AS_SLOT2", "DACC_XDEEP_AS_SLOT2", "DACC_VDEEP_AS_SLOT2", "DACC_LAST_AS_SLOT2"):
        monkeypatch.delenv(name, raising=False)
    wo, fo, bo = fc.oracle("Q"); fc.check("Q", wo)
    E, fe, be = _emul_run(fc.shape("Q"), k=14)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    assert E.counts() == (0, 0, 0, 37), E.counts()


def test_fourth_slot_switch_conflicts_with_each_of_the_others(monkeypatch):
    """DACC_FDEEP_AS_SLOT2=1 names the third slot's main tier like DACC_LAST_AS_SLOT2=1, DACC_VDEEP_AS_SLOT2=1 and DACC_XDEEP_AS_SLOT2=1: with any one of
    them dacc_create returns DACC_EINVAL (before it looks for a device, so this runs without one); alone it passes that check."""
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
    older = ("DACC_LAST_AS_SLOT2", "DACC_VDEEP_AS_SLOT2", "DACC_XDEEP_AS_SLOT2")
    for n in older + ("DACC_FDEEP_AS_SLOT2",):
        monkeypatch.delenv(n, raising=False)
    monkeypatch.setenv("DACC_FDEEP_AS_SLOT2", "1")
    assert create() != EINVAL
    for n in older:
        monkeypatch.setenv(n, "1")
        assert create() == EINVAL, n
        monkeypatch.delenv(n)
    assert create() != EINVAL

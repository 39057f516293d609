"""The wide deep tier (FastTier<19>, daccord_amd/csrc/fast_window.hpp) on the CPU emulation: windows of 251 ... 1000 strings of a WIDE batch
(w = 64 ... 127) leave the generic engine.  The emulation harness walks the slots of the chain only, so the tier is run as the third slot's main tier
(DACC_WDEEP_AS_SLOT2=1: tier 19 in place of tier 9, behind tier 8); without the switch the harness counts what it counted before the stage existed.
Everything equals the oracle bit for bit.  Shapes: tests/wdeep_cases.py.

That the stage is off in a batch without a window of more than 250 strings, in a shallow or deep batch and with DACC_WDEEP_TIER=0 is asserted on the device
through wdeep_ms == 0 (tests/test_gpu_wdeep_tier.py); here the conflict of the slot switches is checked, which dacc_create refuses before it looks for a device."""
import ctypes as C
import numpy as np
import pytest
import emul_lib
import vdeep_cases as vc
import wdeep_cases as wc
from daccord_amd._structs import default_params
from common import windows_equal, frags_equal


def _emul(data, lanes=1, **kw):
    d, ovl, sel = data
    E = emul_lib.Emul(default_params(**kw), lanes=lanes); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fe, be = E.run(sel, ovl, d.trace)
    return E, fe, be


def _generic_list(E):
    """[(window, flags of the tier that handed it on)] of the windows the generic engine ran (tests/emul/emul.cpp: emul_generic_list)"""
    E.L.emul_generic_list.restype = C.c_uint64; E.L.emul_generic_list.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    n = E.L.emul_generic_list(E.h, None, 0); out = np.zeros(n, np.uint64)
    E.L.emul_generic_list(E.h, out.ctypes.data_as(C.c_void_p), n)
    return [(int(w), int(f)) for w, f in out.reshape(-1, 2)]


def _run(name, lanes=1, handed=None):
    """the shape on the emulation, compared with the oracle: (oracle's windows, emulation's windows, counts); `handed` receives the generic list"""
    wo, fo, bo = wc.oracle(name); wc.check(name, wo)
    E, fe, be = _emul(wc.shape(name), lanes=lanes, **wc.params(name))
    we = E.windows()
    assert windows_equal(wo, we) == [] and frags_equal(fo, bo, fe, be)
    if handed is not None:
        handed.extend(_generic_list(E))
    return wo, we, E.counts()


@pytest.mark.parametrize("name,lanes,n", [("WD", 1, 77), ("WD64", 1, 122), ("S251", 1, 62), ("S251", 64, 62), ("S1000", 1, 62)])
def test_deep_wide_windows_finish_in_the_tier(monkeypatch, name, lanes, n):
    """every window finishes in the third slot and none is handed on: a hand-on here is a capacity sized too small"""
    monkeypatch.setenv("DACC_WDEEP_AS_SLOT2", "1")
    wo, we, counts = _run(name, lanes)
    assert counts == (0, 0, n, 0), counts


def test_dense_graph_at_k8_overflows_the_stretch_table(monkeypatch):
    """WD at k = 8 (w = 100: a dense graph) is the one shape the tier is not sized for: 44 of the 77 windows finish in it, 33 are handed on by the stretch
    construction (flag 32: a graph of more than 4000 stretches or 8190 nodes, the most the 12 bit stretch number and the 13 bit node fields of the stretch
    sort key name, FastEngine::QB / KF), and the generic engine finishes those.  The counts are the emulation's; everything equals the oracle."""
    monkeypatch.setenv("DACC_WDEEP_AS_SLOT2", "1")
    wo, we, counts = _run("WD8")
    assert counts == (0, 0, 44, 33), counts


@pytest.mark.parametrize("name,first,deep", [("WM", (0, 3), 53), ("WM8", (0, 7), 81)])
def test_mixed_pile_splits_at_250_strings(monkeypatch, name, first, deep):
    """the windows of more than 250 strings finish in the tier; those of at most 250 that reach it are handed on as they came"""
    monkeypatch.setenv("DACC_WDEEP_AS_SLOT2", "1")
    wo, we, counts = _run(name)
    assert wc.ndeep(wo) == deep
    assert counts[:2] == first and counts[2] == deep, counts
    assert sum(counts) == len(wo)


def test_exactly_250_strings_pass_through(monkeypatch):
    """250 strings are tier 14's side of the seam: tier 19 finishes none and passes all 62 on; tier 14 (DACC_LAST_AS_SLOT2=1) finishes all 62"""
    monkeypatch.setenv("DACC_WDEEP_AS_SLOT2", "1")
    wo, we, counts = _run("S250")
    assert counts == (0, 0, 0, 62), counts
    monkeypatch.delenv("DACC_WDEEP_AS_SLOT2"); monkeypatch.setenv("DACC_LAST_AS_SLOT2", "1")
    wo, we, counts = _run("S250")
    assert counts == (0, 0, 62, 0), counts


@pytest.mark.parametrize("name,over", [("S1001", 9), ("WX", 13)])
def test_more_than_1000_strings_are_handed_on(monkeypatch, name, over):
    """exactly the windows of more than 1000 strings are handed on, each at the string count (generic-list flags 0x3000000, FFAIL(3)); everything else
    finishes in the tier"""
    monkeypatch.setenv("DACC_WDEEP_AS_SLOT2", "1")
    handed = []
    wo, we, counts = _run(name, handed=handed)
    assert wc.nover(wo) == over
    assert counts == (0, 0, len(wo) - over, over), counts
    assert sorted(w for w, f in handed) == [int(i) for i in np.nonzero(wo["mao"] > wc.MAXS)[0]] and len(handed) == over
    assert all(f == 0x3000000 for w, f in handed), sorted(set(hex(f) for w, f in handed))


@pytest.mark.parametrize("name,counts", [("WD", (0, 0, 0, 77)), ("WD64", (0, 0, 0, 122)), ("WM", (0, 3, 4, 95))])
def test_without_the_switch_the_harness_sees_no_new_stage(monkeypatch, name, counts):
    monkeypatch.delenv("DACC_WDEEP_AS_SLOT2", raising=False)
    wo, we, c = _run(name)
    assert c == counts, c


def test_narrow_batch_keeps_tier_3_under_the_switch(monkeypatch):
    """the switch names the third slot's main tier of a wide batch only: shape M of tests/vdeep_cases.py at the default window counts what it counts without it"""
    wo, fo, bo = vc.oracle("M"); vc.check("M", wo)
    monkeypatch.delenv("DACC_WDEEP_AS_SLOT2", raising=False)
    E0, f0, b0 = _emul(vc.shape("M"), k=14)
    monkeypatch.setenv("DACC_WDEEP_AS_SLOT2", "1")
    E, fe, be = _emul(vc.shape("M"), k=14)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    assert E.counts() == E0.counts() == (23, 5, 0, 131), (E0.counts(), E.counts())


def test_slot_switches_together_are_refused(monkeypatch):
    """DACC_WDEEP_AS_SLOT2=1 and DACC_LAST_AS_SLOT2=1 both name the third slot's main tier: dacc_create returns DACC_EINVAL (before it looks for a
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
    monkeypatch.setenv("DACC_LAST_AS_SLOT2", "1"); monkeypatch.setenv("DACC_WDEEP_AS_SLOT2", "1")
    assert create() == EINVAL
    monkeypatch.delenv("DACC_LAST_AS_SLOT2")
    assert create() != EINVAL
    monkeypatch.delenv("DACC_WDEEP_AS_SLOT2"); monkeypatch.setenv("DACC_LAST_AS_SLOT2", "1")
    assert create() != EINVAL


def test_timing_record_grows_by_16_bytes():
    from daccord_amd._structs import DaccTiming, DaccTimingLong, DaccTimingFull, DaccTimingWide
    assert (C.sizeof(DaccTiming), C.sizeof(DaccTimingLong), C.sizeof(DaccTimingFull), C.sizeof(DaccTimingWide)) == (176, 192, 208, 224)
    assert (DaccTimingWide.wdeep_ms.offset, DaccTimingWide.wdeep_windows.offset, DaccTimingWide.wdeep_out.offset) == (208, 212, 216)
    assert DaccTimingWide.fdeep_ms.offset == DaccTimingFull.fdeep_ms.offset == 192

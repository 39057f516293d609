"""The device-memory tiers (FastTier<13> / FastTier<14>, daccord_amd/csrc/fast_window.hpp: the last stage of the tier chain, ID_LAST of
tier_pipeline.hpp) on the CPU emulation.  The emulation harness (tests/emul/emul.cpp) runs the slots of the chain and knows no last stage;
DACC_LAST_AS_SLOT2=1 makes tier 13 (wide batches: 14) the main tier of the third slot, which the harness does run.  Everything equals the
oracle bit for bit on every route, and without the switch the harness counts what it counted before the stage existed.

Counts: Emul.counts() = windows finished by the main tiers of the three slots and by the generic engine."""
import pytest
import emul_lib
import last_tier_cases as LC
from common import windows_equal, frags_equal

# what the chain does with the shapes without the switch (the counts from before the last stage): (slot 0, slot 1, slot 2, generic engine), tier 10
BEFORE = {"A": ((33, 246, 0, 0), 29), "W": ((0, 1174, 66, 0), 0), "H": ((20, 378, 87, 10), 2)}


def _emul(name, lanes=1):
    d, ovl, sel = LC.shape(name)
    E = emul_lib.Emul(LC.params(name), lanes=lanes); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fe, be = E.run(sel, ovl, d.trace)
    return E, fe, be


def _equal(name, E, fe, be):
    wo, fo, bo = LC.oracle(name)
    return windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)


@pytest.mark.parametrize("name", ["A", "W", "H"])
def test_without_the_switch_the_harness_counts_as_before(name, monkeypatch):
    monkeypatch.delenv("DACC_LAST_AS_SLOT2", raising=False)
    E, fe, be = _emul(name)
    assert _equal(name, E, fe, be)
    assert (E.counts(), E.count_tier10()) == BEFORE[name]


@pytest.mark.parametrize("name,lanes", [("A", 1), ("A", 64), ("W", 1), ("W", 64)])
def test_default_chain_with_the_tier_as_third_slot(name, lanes, monkeypatch):
    """the third slot finishes what tier 3 / tier 9 finish without the switch: the capacities include theirs"""
    monkeypatch.setenv("DACC_LAST_AS_SLOT2", "1")
    E, fe, be = _emul(name, lanes)
    assert _equal(name, E, fe, be)
    assert (E.counts(), E.count_tier10()) == BEFORE[name] and E.counts()[3] == 0


@pytest.mark.parametrize("lanes", [1, 64])
def test_narrow_tier_takes_the_first_slots_hand_overs(lanes, monkeypatch):
    """DACC_TIERS=29: first and third slot only, so tier 13 reads all 275 windows the first slot hands on in shape A (the windows the last stage
    reads on the device under DACC_TIERS=25) and finishes every one -- its capacities include tier 6's, tier 10's and tier 3's."""
    monkeypatch.setenv("DACC_LAST_AS_SLOT2", "1"); monkeypatch.setenv("DACC_TIERS", "29")
    E, fe, be = _emul("A", lanes)
    assert _equal("A", E, fe, be)
    assert E.counts() == (33, 0, 275, 0)


def test_wide_tier_takes_tier_8s_place(monkeypatch):
    """DACC_TIERS=4: the third slot alone, so tier 14 runs every window of the wide shape, including the 1174 tier 8 finishes by default"""
    monkeypatch.setenv("DACC_LAST_AS_SLOT2", "1"); monkeypatch.setenv("DACC_TIERS", "4")
    E, fe, be = _emul("W")
    assert _equal("W", E, fe, be)
    assert E.counts() == (0, 0, 1240, 0)


def test_capacity_shape_finishes_in_the_tier(monkeypatch):
    """Shape H: the ten windows that overflow tier 3's weight table (8193 forward weight records against 8192) and ended in the generic engine
    finish in tier 13, whose weight table holds 16384 records per direction: 16 bit weight offsets are enough for all ten."""
    monkeypatch.setenv("DACC_LAST_AS_SLOT2", "1")
    E, fe, be = _emul("H")
    assert _equal("H", E, fe, be)
    before = BEFORE["H"][0]
    finished = E.counts()[2] - before[2]
    assert finished >= 8 and finished == LC.H_FINISHED
    assert E.counts() == (before[0], before[1], before[2] + finished, before[3] - finished)
    wo = LC.oracle("H")[0]
    assert ((wo["status"][list(LC.H_WINDOWS)] == 1) & (wo["filterfreq"][list(LC.H_WINDOWS)] == 1)).all()

"""The long string stage (FastTier<17>, daccord_amd/csrc/fast_window.hpp: ID_LONG of a wide batch, tier_pipeline.hpp) on the CPU emulation: the
windows of a wide batch (w = 64 ... 127) with a B string of more than 128 bases, which the pre-scan puts on the second stream's list, run in a
tier with four words per pattern mask (strings of up to 255 bases) in front of the generic engine.  The emulation harness (tests/emul/emul.cpp)
runs its ROLE_LONG stage over that list with one buffer and no slab, which is how the tier keeps its working set (FastTier<17>::oneslab).
Everything equals the oracle bit for bit with the stage and without it (DACC_LONGSTR_TIER=0), and without it the harness counts what it counted
before the stage existed.  Shapes: tests/longstr_cases.py.

Counts: Emul.counts() = windows finished by the main tiers of the three slots and by the generic engine (which here also takes what the last
stage takes on the device: the harness walks the slots only); Emul.count_long() = windows finished by the second stream's tier.

What the stage hands on (DACC_EMUL_OVER=1 names the place): N120, W64 and S nothing; N127 two of 194 windows at the reverse path cache (flags
0x4200: 4096 paths, tier 14's rccap); S2 the window with a string of 256 bases (code 4, too long); W100 none of its list of 20.  Tier 14's own
tables sent on 21 of N120's 73 and 55 of N127's 194: 15 / 43 at the gap filling scratch -- which in tier 14's layout has no room at all, the build
overlay being the longer one -- and 6 / 12 at the forward pool (512 paths per first k-mer, flags 0x10200); tier 17 has a gap filling scratch of
its own (16384 records) and a forward pool of 4096 paths in up to 64 chunks per first k-mer."""
import ctypes as C
import numpy as np
import pytest
import pyoracle
import emul_lib
import longstr_cases as LC
from common import windows_equal, frags_equal

# (slot 0, slot 1, slot 2, generic engine) without the stage: the counts from before it, count_long() == 0
BEFORE = {"N120": (0, 126, 92, 73), "N127": (0, 52, 27, 194), "W64": (0, 261, 34, 15), "W100": (0, 18, 149, 30), "W96": (0, 296, 70, 0),
          "S": (0, 38, 17, 4), "S2": (0, 4, 6, 37)}
FINISHED = LC.FINISHED      # windows that finish in the stage

_runs = {}


def _generic_list(E):
    """[(window, flags of the tier that handed it on)] of the windows the generic engine ran"""
    E.L.emul_generic_list.restype = C.c_uint64; E.L.emul_generic_list.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    n = E.L.emul_generic_list(E.h, None, 0); out = np.zeros(n, np.uint64)
    E.L.emul_generic_list(E.h, out.ctypes.data_as(C.c_void_p), n)
    return [(int(w), int(f)) for w, f in out.reshape(-1, 2)]


def _emul(name, stage, monkeypatch, lanes=1):
    """one emulation run per (shape, switch, lanes) and process: (counts, count_long, generic list, windows, fragments, bases)"""
    key = (name, stage, lanes)
    if key not in _runs:
        for k in ("DACC_TIERS", "DACC_LAST_AS_SLOT2", "DACC_WIDE_TIER", "DACC_LONGSTR_TIER"):
            monkeypatch.delenv(k, raising=False)
        if not stage:
            monkeypatch.setenv("DACC_LONGSTR_TIER", "0")
        d, ovl, sel, tr, tb = LC.shape(name)
        E = emul_lib.Emul(LC.params(name), lanes=lanes); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
        fe, be = E.run(sel, ovl, tr, trace_bytes=tb)
        _runs[key] = (E.counts(), E.count_long(), _generic_list(E), E.windows(), fe, be)
    return _runs[key]


def _equal(name, run):
    wo, fo, bo = LC.oracle(name)
    LC.check(name, wo)
    return windows_equal(wo, run[3]) == [] and frags_equal(fo, bo, run[4], run[5])


@pytest.mark.parametrize("name", ["N120", "N127", "W64", "W100", "W96", "S", "S2"])
def test_equals_the_oracle_with_the_stage(name, monkeypatch):
    assert _equal(name, _emul(name, True, monkeypatch))


def test_equals_the_oracle_with_64_lanes(monkeypatch):
    run = _emul("W64", True, monkeypatch, lanes=64)
    assert _equal("W64", run)
    assert (run[0], run[1]) == _emul("W64", True, monkeypatch)[:2]


@pytest.mark.parametrize("name", ["N120", "N127", "W64", "W100"])
def test_the_stage_finishes_windows(name, monkeypatch):
    """fails without the feature: no tier of a wide batch's second stream existed, count_long() was 0 for every wide batch"""
    assert _emul(name, True, monkeypatch)[1] > 0


@pytest.mark.parametrize("name", ["N120", "N127", "W64", "W100", "W96", "S", "S2"])
def test_switch_off_counts_as_before_and_no_other_route_moves(name, monkeypatch):
    off = _emul(name, False, monkeypatch); on = _emul(name, True, monkeypatch)
    assert _equal(name, off)
    assert (off[0], off[1]) == (BEFORE[name], 0)
    assert on[0][:3] == off[0][:3]                      # the slots finish what they finished
    assert on[1] + on[0][3] == off[0][3]                # every window of the generic engine's is finished once: in the stage or there
    assert on[1] == FINISHED[name]
    assert sum(off[0]) == len(off[3]) and sum(on[0]) + on[1] == len(on[3])
    # the generic engine runs a subset of what it ran
    assert set(w for w, _ in on[2]) <= set(w for w, _ in off[2])


@pytest.mark.parametrize("name", ["N120", "N127", "W64"])
def test_the_stage_finishes_three_quarters_of_the_prescan_list(name, monkeypatch):
    """the lists hold no string near 255 bases and the other windows of these shapes fit tier 14's tables"""
    off = _emul(name, False, monkeypatch); on = _emul(name, True, monkeypatch)
    n = LC.LISTLEN[name]
    assert off[0][3] == n               # in these shapes the slots hand nothing on: what the generic engine ran without the stage is the list
    print("%s: list %d, finished in the stage %d, handed on %s" % (name, n, on[1], [(w, hex(f)) for w, f in on[2]]))
    assert 4 * on[1] >= 3 * n
    assert on[1] == FINISHED[name]


def test_no_long_string_no_stage(monkeypatch):
    on = _emul("W96", True, monkeypatch)
    assert (on[0], on[1]) == (BEFORE["W96"], 0) and LC.LISTLEN["W96"] == 0


def test_seam_128_stays_in_the_slots_129_and_255_finish_in_the_stage(monkeypatch):
    sw = LC.seam_windows("S")
    off = _emul("S", False, monkeypatch); on = _emul("S", True, monkeypatch)
    assert _equal("S", off) and _equal("S", on)
    listed = set(w for w, _ in off[2])      # without the stage the generic engine runs the pre-scan list (the slots hand nothing on here: below)
    assert off[0][3] == len(listed) == 4
    assert sw[128] not in listed            # a string of 128 bases: the slots' tiers hold it, the window is not on the second stream's list
    assert sw[129] in listed and sw[255] in listed
    assert on[2] == [] and on[1] == 4       # all of the list finishes in the stage
    bl = LC.block_lengths("S")
    assert sorted(int(v) for v in bl[bl >= 128]) == [128, 129, 255]


def test_seam_255_finishes_in_the_stage_256_goes_to_the_generic_engine(monkeypatch):
    sw = LC.seam_windows("S2")
    off = _emul("S2", False, monkeypatch); on = _emul("S2", True, monkeypatch)
    assert _equal("S2", off) and _equal("S2", on)
    listed = set(w for w, _ in off[2])
    assert sw[255] in listed and sw[256] in listed
    assert on[2] == [(sw[256], 4 << 24)]    # handed on at the length check (FFAIL(4): FW_GENERIC) before anything was built
    assert on[1] == len(listed) - 1
    bl = LC.block_lengths("S2")
    assert int(bl.max()) == 256 and int((bl == 255).sum()) == 1


@pytest.mark.parametrize("name", ["N120", "W64", "S", "S2"])
def test_fasta_identical_with_and_without_the_stage(name, monkeypatch):
    off = _emul(name, False, monkeypatch); on = _emul(name, True, monkeypatch)
    fa = pyoracle.fasta(on[4], on[5])
    assert fa == pyoracle.fasta(off[4], off[5]) == pyoracle.fasta(*LC.oracle(name)[1:]) and len(fa) > 1000

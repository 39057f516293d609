"""The tier of w = 128 (FastTier<20>, daccord_amd/csrc/fast_window.hpp) on the CPU emulation: position masks of three 64 bit words (the model table of
w = 128 has 129 rows), candidates and a consensus of up to 192 symbols, strings of up to 255 bases.  On the device the tier is the one stage of a batch with
w = 128 (tier_pipeline.hpp: ID_W128), in front of the generic engine; the emulation harness walks the three slots and the second stream's stage only, so the
tier is run there under DACC_W128_AS_SLOT2=1: the third slot's main tier (windows whose strings have at most 128 bases, with a slab) and the second stream's
tier (windows with a longer string, in one buffer).  Everything equals the oracle bit for bit.  Without the switch the emulation of a w = 128 batch is the
generic engine alone, as before the tier.  Shapes: tests/w128_cases.py.

Counts: Emul.counts() = windows finished by the main tiers of the three slots and by the generic engine; Emul.count_long() = windows finished by the second
stream's tier.  What the tier hands on (measured): A, D, E and K nothing; the seam shape the windows with a string of more than 255 bases (code 4)."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import pyoracle
import emul_lib
import w128_cases as WC
from common import windows_equal, frags_equal

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "daccord_amd", "csrc")
_SWITCHES = ("DACC_TIERS", "DACC_LAST_AS_SLOT2", "DACC_WDEEP_AS_SLOT2", "DACC_WIDE_TIER", "DACC_LONGSTR_TIER", "DACC_W128_TIER", "DACC_W128_AS_SLOT2", "DACC_NOFAST")
_runs = {}


def _generic_list(E):
    """[(window, flags of the tier that handed it on)] of the windows the generic engine ran"""
    E.L.emul_generic_list.restype = C.c_uint64; E.L.emul_generic_list.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    n = E.L.emul_generic_list(E.h, None, 0); out = np.zeros(n, np.uint64)
    E.L.emul_generic_list(E.h, out.ctypes.data_as(C.c_void_p), n)
    return [(int(w), int(f)) for w, f in out.reshape(-1, 2)]


def _emul(name, switch, monkeypatch, lanes=1):
    """one emulation run per (shape, switch, lanes) and process: (counts, count_long, generic list, windows, fragments, bases)"""
    key = (name, switch, lanes)
    if key not in _runs:
        for k in _SWITCHES:
            monkeypatch.delenv(k, raising=False)
        if switch:
            monkeypatch.setenv("DACC_W128_AS_SLOT2", "1")
        d, ovl, sel, tr, tb = WC.shape(name)
        E = emul_lib.Emul(WC.params(name), lanes=lanes); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
        fe, be = E.run(sel, ovl, tr, trace_bytes=tb)
        _runs[key] = (E.counts(), E.count_long(), _generic_list(E), E.windows(), fe, be)
    return _runs[key]


def _equal(name, run):
    wo, fo, bo = WC.oracle(name)
    WC.check(name, wo)
    return windows_equal(wo, run[3]) == [] and frags_equal(fo, bo, run[4], run[5]) and pyoracle.fasta(run[4], run[5]) == pyoracle.fasta(fo, bo)


@pytest.mark.parametrize("name,lanes", [("A", 1), ("D", 1), ("D", 64), ("E", 1), ("K", 1), ("S", 1)])
def test_equals_the_oracle_in_the_tier(name, lanes, monkeypatch):
    run = _emul(name, True, monkeypatch, lanes)
    assert _equal(name, run)
    if lanes == 64:
        assert run[:3] == _emul(name, True, monkeypatch)[:3]


@pytest.mark.parametrize("name", ["A", "D", "E"])
def test_the_tier_finishes_its_windows(name, monkeypatch):
    """fails without the tier: no slot and no second stream's tier was resolved for w = 128, every window ran in the generic engine.  The generic
    engine runs at most 5 % of the windows of each shape -- a condition on the tier's capacities, not a measurement"""
    counts, nlong, handed, we, fe, be = _emul(name, True, monkeypatch)
    n = len(we)
    print("w128 %s: %d windows, slot path %d, second-stream path %d, generic engine %d %s" % (name, n, counts[2], nlong, counts[3], sorted(set(hex(f) for w, f in handed))))
    assert counts[0] == counts[1] == 0 and counts[2] + nlong + counts[3] == n
    assert counts[2] + nlong > 0
    assert 20 * counts[3] <= n
    assert len(handed) == counts[3]


def test_premises_of_the_shapes(monkeypatch):
    """so that no test passes empty: windows with a consensus in A, consensus of more than 128 symbols in D and E (the rows of 192 symbols), and in A both
    paths -- windows whose strings have at most 128 bases on the slot path, windows with a longer string on the second stream's"""
    wa = WC.oracle("A")[0]; wd = WC.oracle("D")[0]; we = WC.oracle("E")[0]
    assert int((wa["status"] == 1).sum()) >= 250
    assert int(((wd["status"] == 1) & (wd["conslen"] > 128)).sum()) >= 250
    assert int(((we["status"] == 1) & (we["conslen"] > 128)).sum()) >= 100
    counts, nlong = _emul("A", True, monkeypatch)[:2]
    assert nlong > 0 and counts[2] > 0
    # the long consensus windows finish in the tier, not in the generic engine behind it
    for name, wo in (("D", wd), ("E", we)):
        handed = set(w for w, f in _emul(name, True, monkeypatch)[2])
        longc = [i for i in np.nonzero((wo["status"] == 1) & (wo["conslen"] > 128))[0] if int(i) not in handed]
        assert len(longc) >= (250 if name == "D" else 100)


def test_seam_128_129_255_finish_in_the_tier_256_goes_to_the_generic_engine(monkeypatch):
    sw = WC.seam_windows()
    on = _emul("S", True, monkeypatch)
    assert _equal("S", on)
    handed = dict(on[2])
    assert sw[128] not in handed and sw[129] not in handed and sw[255] not in handed
    assert handed.get(sw[256]) == 4 << 24            # handed on at the length check (FFAIL(4): FW_GENERIC) before anything was built
    assert all(f == 4 << 24 for f in handed.values()), sorted(set(hex(f) for f in handed.values()))      # (its half-overlapping neighbours may have such a string too)
    assert on[0][2] + on[1] == len(on[3]) - len(handed) and on[0][3] == len(handed) <= 3
    bl = WC.block_lengths("S")
    assert int(bl.max()) == 256 and int((bl == 255).sum()) == 1


def test_without_the_switch_the_generic_engine_alone(monkeypatch):
    off = _emul("S", False, monkeypatch)
    assert _equal("S", off)
    assert off[0] == (0, 0, 0, len(off[3])) and off[1] == 0


def _resolution(tmp_path, env, nrows=129, nsup=166):
    exe = str(tmp_path / "w128_resolution")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-isystem", _CSRC, "-o", exe, os.path.join(_HERE, "tiers", "w128_resolution.cpp")])
    e = {k: v for k, v in os.environ.items() if not k.startswith("DACC_")}
    e.update(env)
    r = subprocess.run([exe, str(nrows), str(nsup)], capture_output=True, timeout=300, env=e)
    assert r.returncode == 0 and b"runtime error" not in r.stderr, r.stderr.decode()[-2000:]
    return r.stdout.decode().strip()


def test_resolution_of_the_stage_with_all_rows(tmp_path):
    """resolveTiers with rows = TIER_NROWS, as the library calls it.  A line: conflict usefast widetier anytier | ok, tier of ID_W128, ID_SLOT2, ID_LONG |
    other rows that are ok || the same for a wide batch of w = 100, which no switch of the stage moves"""
    W100 = "0 1 1 1 | 0 20 1 9 1 17 | 2"      # tier 8, tier 9, the long string stage; the last stage: slots 1 and 2 and ID_LAST beside ID_SLOT2 and ID_LONG
    # default: the stage alone
    assert _resolution(tmp_path, {}) == "0 1 1 0 | 1 20 0 9 0 17 | 0 || " + W100
    # switched off: nothing resolved, the generic engine alone as before the stage
    assert _resolution(tmp_path, {"DACC_W128_TIER": "0"}) == "0 1 1 0 | 0 20 0 9 0 17 | 0 || " + W100
    # the test switch: the tier as the third slot's main tier and as the second stream's tier, the stage off, no other row
    assert _resolution(tmp_path, {"DACC_W128_AS_SLOT2": "1"}) == "0 1 1 1 | 0 20 1 20 1 20 | 0 || " + W100
    # it takes part in the conflict of the slot switches
    assert _resolution(tmp_path, {"DACC_W128_AS_SLOT2": "1", "DACC_LAST_AS_SLOT2": "1"}).startswith("1 ")
    # wide tiers off, the fast path off: no stage
    assert _resolution(tmp_path, {"DACC_WIDE_TIER": "0"}).startswith("0 0 0 0 | 0 20 0 9 0 17 | 0 || ")
    assert _resolution(tmp_path, {"DACC_NOFAST": "1"}).startswith("0 0 1 0 | 0 20 0 9 0 17 | 0 || ")
    # a model table of more rows than three mask words name, or more read offsets than the wide table copy holds: no stage
    assert _resolution(tmp_path, {}, nrows=193).startswith("0 0 0 0 | 0 ")
    assert _resolution(tmp_path, {}, nsup=193).startswith("0 0 0 0 | 0 ")
    assert _resolution(tmp_path, {}, nrows=192, nsup=192).startswith("0 1 1 0 | 1 20 ")


def test_layout_of_the_tier_is_the_recorded_one(tmp_path):
    """tier 20 stands in a tier list of its own (DACC_W128_TIERS, tier_pipeline.hpp), beside the lists whose layouts tests/golden/fast_layout_sizes.txt records:
    its line is recorded here, and the kernel lists that the launches walk hold it"""
    exe = str(tmp_path / "w128_layout_sizes")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-isystem", _CSRC, "-o", exe, os.path.join(_HERE, "tiers", "w128_layout_sizes.cpp")])
    r = subprocess.run([exe], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"runtime error" not in r.stderr
    assert r.stdout == open(os.path.join(_HERE, "golden", "w128_layout_sizes.txt"), "rb").read() and r.stdout.startswith(b"tier 20 ")
    hdr = open(os.path.join(_CSRC, "tier_pipeline.hpp")).read()
    assert "#define DACC_W128_TIERS(X) X(20)" in hdr and "#define DACC_EVERY_KERNEL_TIER(X) DACC_KERNEL_TIERS(X) DACC_W128_TIERS(X)" in hdr


def test_model_tables_of_w128_fit_the_wide_table_copy():
    """FSUPCAPW = 192 read offsets: the tables of the test profiles, of a narrow profile (0.03, 0.01, 0.95) and of a wide one at w = 128"""
    from daccord_amd._structs import default_params
    seen = {}
    for key, prof in [(n, WC.shape(n)[0].error_profile()) for n in "ADE"] + [("narrow", (0.03, 0.01, 0.95)), ("wide", (0.2, 0.05, 0.7))]:
        E = emul_lib.Emul(default_params(k=12, w=128, a=32)); E.set_error_profile(*prof); t = E.tables()
        seen[key] = (int(t[0]), int(t[1]))
    print("w128 model tables (rows, read offsets):", seen)
    assert all(r == 129 and s <= 192 for r, s in seen.values()), seen


def test_timing_record_grows_by_16_bytes():
    from daccord_amd._structs import DaccTiming, DaccTimingLong, DaccTimingFull, DaccTimingWide, DaccTimingW128
    assert tuple(C.sizeof(t) for t in (DaccTiming, DaccTimingLong, DaccTimingFull, DaccTimingWide, DaccTimingW128)) == (176, 192, 208, 224, 240)
    assert (DaccTimingW128.w128_ms.offset, DaccTimingW128.w128_windows.offset, DaccTimingW128.w128_out.offset, DaccTimingW128.pad5_.offset) == (224, 228, 232, 236)
    assert DaccTimingW128.wdeep_ms.offset == DaccTimingWide.wdeep_ms.offset == 208

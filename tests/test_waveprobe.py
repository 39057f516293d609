"""The wavefront primitives of daccord_amd/csrc/wave.hpp, one at a time, against numpy -- on the 64-lane host wavefront
(tests/waveprobe/probe_host.cpp).  No GPU: this validates the probe bodies and the expected values of tests/waveprobe_cases.py, and holds
wave_emul64.hpp's restatements of the primitives to the table that tests/test_gpu_waveprobe.py holds the device branch to."""
import os
import re
import numpy as np
import pytest
import waveprobe_lib as WL
import waveprobe_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    return WL.Probe("host")


def _pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def test_probe_sorts_what_the_product_instantiates(P):
    """the (CAP, R32) pairs of wv_sort_keys, read off the FastTier table (fast_tiers.hpp) and the engine's calls (fast_window.hpp:
    wv_sort_keys<keycap>, <precap[,R32]>, <fcpow2(scap)>)"""
    src = "".join(open(os.path.join(ROOT, "daccord_amd", "csrc", f)).read() for f in ("fast_tiers.hpp", "fast_window.hpp"))
    defs = dict(re.findall(r"^#define\s+(\w+)\s+(\d+)\s*$", src, re.M))
    tiers = re.findall(r"template<> struct FastTier<(\d+)> \{[^\n]*?enum : uint32_t \{([^}]*)\}", src)
    assert len(tiers) >= 15
    want = set()
    for _, body in tiers:
        f = {k: int(defs.get(v, v)) for k, v in re.findall(r"(\w+) = (\w+)", body) if defs.get(v, v).isdigit()}
        want |= {(_pow2(max(f["maxs"], 2)), False), (f["precap"], False), (_pow2(f["scap"]), False)}
        if f["precap"] == 2048 and f["ncap"] == 256:
            want.add((2048, True))
    calls = set(re.findall(r"wv_sort_keys<([^;]*?)>\(L\.", src))
    assert calls == {"FastLds<CT>::keycap", "CT::precap,(CT::precap == 2048 && CT::ncap == 256)", "CT::precap", "fcpow2(CT::scap)"}, calls
    assert set(WC.SORT_PAIRS) == want and len(set(WC.SORT_PAIRS)) == len(WC.SORT_PAIRS)
    assert P.sort_pairs() == WC.SORT_PAIRS
    assert max(c for c, _ in WC.SORT_PAIRS) == WC.MAXN


def test_case_table_has_the_seams():
    names, V, F = WC.u32_cases()
    for s in WC.SEAMS:
        assert any(n.startswith("single@%d/" % s) for n in names) and any(n.endswith("/flag@%d" % s) for n in names)
    assert any((v == 0).all() for v in V) and any((v == WC.M32).all() for v in V) and any((v >> 31).all() for v in V)
    assert any(f.all() for f in F) and any(not f.any() for f in F)
    for mode in range(WC.NMODES):
        sizes = WC.sort_sizes(mode)
        if mode < len(WC.SORT_PAIRS):
            cap = WC.SORT_PAIRS[mode][0]
            assert sizes[-1] == cap and cap - 1 in sizes and all(n in sizes for n in WC.SORT_SIZES if n <= cap)
    assert set(WC.sort_sizes(WC.MODE_BITONIC_N)) >= set(WC.SORT_SIZES) | {WC.MAXN - 1, WC.MAXN}


def test_scans_reductions_votes_32(P):
    WC.check_u32(P)


def test_reductions_64(P):
    WC.check_u64(P)


def test_broadcasts_and_shuffles(P):
    WC.check_xlane(P)


@pytest.mark.parametrize("space", [WL.SPACE_LDS, WL.SPACE_GLOBAL], ids=["lds", "global"])
@pytest.mark.parametrize("mode", range(WC.NMODES), ids=WC.mode_name)
def test_sorts(P, mode, space):
    WC.check_sort(P, mode, space)


@pytest.mark.parametrize("space", [WL.SPACE_LDS, WL.SPACE_GLOBAL], ids=["lds", "global"])
def test_index_sort_with_pads_and_ties(P, space):
    WC.check_sort_idx(P, space)


@pytest.mark.parametrize("init", [0, 0xFFFFFF00])
def test_atomic_adds(P, init):
    WC.check_atomic(P, init)


def test_entry_points_refuse_jobs_outside_their_buffers(P):
    """nothing is launched on a job that would touch memory outside the key buffer, beyond its mode's capacity, or (bitonic) not a power of two"""
    keys = np.zeros(64, np.uint64)
    for job in [(0, 33, 0, 0), (0, 32, 40, 0), (WC.NMODES, 8, 0, 0), (WC.MODE_BITONIC, 24, 0, 0), (WC.MODE_BITONIC_N, 65, 0, 0)]:
        with pytest.raises(WL.ProbeError):
            P.sort(WL.SPACE_GLOBAL, np.array([job], WL.JOB), keys)
    with pytest.raises(WL.ProbeError):
        P.sort_idx(WL.SPACE_LDS, np.array([(4, 2, 0, 0)], WL.IDXJOB), np.zeros(2, np.uint64), np.array([0, 1, 2, 0xFFFFFFFF], np.uint32))
    names, v32, v64, src, bsrc = WC.xlane_cases()
    with pytest.raises(WL.ProbeError):
        P.xlane(v32[:1], v64[:1], src[:1] + 64, bsrc[:1])

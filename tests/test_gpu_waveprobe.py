"""The DEVICE branch of daccord_amd/csrc/wave.hpp -- DPP scans (row_shr, row_bcast15 / 31, readlane 63), ballot + mbcnt, readlane /
readfirstlane broadcasts, __shfl / __shfl_xor, the register sorts and the bitonic networks on LDS and on global pointers, the atomics --
one primitive at a time against numpy, on gfx950 (tests/waveprobe/probe.hip, compiled with the product's flags).  The case table is the
one tests/test_waveprobe.py runs on the host wavefront (tests/waveprobe_cases.py).  A HIP error of an entry point fails the test with its text."""
import pytest
import waveprobe_lib as WL
import waveprobe_cases as WC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return WL.Probe("dev")


def test_probe_holds_the_products_sort_instantiations(P):
    assert P.sort_pairs() == WC.SORT_PAIRS


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

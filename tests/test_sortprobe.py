"""The engines' replays of libstdc++'s std::sort on the reverse paths of a window (comparator (front, baselen); the permutation of tied keys is part
of the result), probed one call at a time on chosen keys (tests/sortprobe/sortprobe.cpp, host code, compiled on demand): WindowEngine::arpSort of the
generic engine, which reproduces introsort's heapsort fallback at the depth limit 2 * floor(log2 n), and the two copies of the tiers (arpSort on
ids, arpSortK on (id, key) pairs; probed as tier 3 with 16 bit ids and tier 1 with 8 bit ids), which refuse such a block with flag 1024 and hand
the window on.  Expected: std::sort over an array of structs with the same comparator, compiled into the probe.

Killer inputs are made by McIlroy's adversary playing against that std::sort with tied keys (`copies` equal keys per value).  The depth limit can
only be reached from 37 keys on: a median-of-3 pivot leaves at most n - 2 keys in the larger part, and a range of at most 16 is left to the
final insertion sort, so the limit needs n - 4 * floor(log2 n) > 16.  The killers of 17, 32 and 33 keys therefore must NOT take the fallback."""
import numpy as np
import pytest
import sortprobe_lib as sp

CAP = sp.capacity(sp.GENERIC)
# (n, mirror, copies): a few distinct fronts and lengths wherever the size allows
KILLERS = [(64, 0, 1), (64, 1, 2), (100, 0, 2), (100, 1, 2), (1000, 0, 7), (1000, 1, 2), (4096, 0, 32), (4096, 1, 2), (CAP, 0, 8192), (CAP, 0, 2048), (CAP, 1, 4)]
TOO_SMALL = [(n, m, c) for n in (17, 32, 33) for m in (0, 1) for c in (1, 2, 4)]


def keys_of(q):
    """16 base lengths per front k-mer"""
    q = np.asarray(q, np.uint64)
    return (1000 + q // 16).astype(np.uint32), (12 + q % 16).astype(np.uint16)


def run_all(front, baselen):
    """the generic engine equals std::sort; a tier that takes the block equals it too, and refuses exactly where the generic engine fell back"""
    want = sp.expected(front, baselen)
    assert sorted(want.tolist()) == list(range(len(front)))
    got, flags, fb = sp.sort(sp.GENERIC, front, baselen)
    assert flags == 0 and np.array_equal(got, want)
    for e in sp.TIERS:
        if len(front) <= sp.capacity(e):
            g, f, _ = sp.sort(e, front, baselen)
            assert f == (sp.REFUSED if fb else 0), (e, f, fb)
            assert f or np.array_equal(g, want), e
    return fb


def test_capacities():
    assert CAP == 8192 * 4 ** 3 and [sp.capacity(e) for e in sp.TIERS] == [2048, 2048, 144, 144]
    with pytest.raises(ValueError):
        sp.sort(sp.TIER1, np.zeros(145, np.uint32), np.zeros(145, np.uint16))


@pytest.mark.parametrize("n,mirror,copies", KILLERS)
def test_killer_sequences_take_the_fallback(n, mirror, copies):
    q = sp.killer(n, mirror, copies)
    assert len(np.unique(q)) == (n + copies - 1) // copies
    assert run_all(*keys_of(q)) >= 1


@pytest.mark.parametrize("n,mirror,copies", TOO_SMALL)
def test_fewer_than_37_keys_never_reach_the_depth_limit(n, mirror, copies):
    assert n - 4 * (n.bit_length() - 1) <= 16
    assert run_all(*keys_of(sp.killer(n, mirror, copies))) == 0


@pytest.mark.parametrize("n", [0, 1, 2, 15, 16, 17, 32, 33, 64, 100, 144, 145, 1000, 2048, 4096, CAP])
def test_sorted_reversed_and_equal_keys(n):
    for d in (1, 3, 40):      # distinct keys
        up = (np.arange(n, dtype=np.uint64) * d) // max(n, 1)
        assert run_all(*keys_of(up)) == 0
        assert run_all(*keys_of(up[::-1])) == 0
    # organ pipe and saw tooth
    assert run_all(*keys_of(np.minimum(np.arange(n), np.arange(n)[::-1]) % 48)) == 0
    run_all(*keys_of(np.arange(n) % 7))


@pytest.mark.parametrize("n", [17, 32, 33, 64, 100, 1000, 4096, CAP])
def test_random_keys_do_not_take_the_fallback(n):
    rs = np.random.RandomState(n)
    for d in (2, 9, 64, 256):
        assert run_all(*keys_of(rs.randint(0, d, size=n))) == 0
    # fronts and lengths drawn apart: ties in the front alone, in the length alone, in both
    fr = rs.randint(0, 5, size=n).astype(np.uint32) * 4097; bl = rs.randint(12, 20, size=n).astype(np.uint16)
    assert run_all(fr, bl) == 0


def test_base_lengths_beyond_a_byte_in_the_generic_engine():
    """the generic engine's base lengths are 16 bit (w = 128 makes paths beyond 255 bases); the tiers' are 8 bit and the probe refuses such keys"""
    rs = np.random.RandomState(5)
    fr = rs.randint(0, 3, size=500).astype(np.uint32); bl = rs.randint(200, 400, size=500).astype(np.uint16)
    got, flags, fb = sp.sort(sp.GENERIC, fr, bl)
    assert flags == 0 and np.array_equal(got, sp.expected(fr, bl))
    with pytest.raises(ValueError):
        sp.sort(sp.TIER3, fr, bl)

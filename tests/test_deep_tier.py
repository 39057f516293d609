"""The deep-window tier (FastTier<12>, daccord_amd/csrc/fast_window.hpp) on the CPU emulation: windows of 97 ... 250 strings -- repeat piles --
finish in an LDS tier of their own, in front of tier 3, instead of the generic engine; deeper windows still go there, and DACC_DEEP_TIER=0
restores that route for all of them.  Everything equals the oracle bit for bit.

The emulation (tests/emul/emul.cpp) walks the tier chain generically and keeps no counter for the stage, so the tier's count is inferred:
windows - (tier 0 + tier 7 + tier 10 / 11 + the three slots + tier 5 + generic engine)."""
import pytest
import pyoracle
import emul_lib
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData
from common import windows_equal, frags_equal

MINS, MAXS = 96, 250      # FastTier<12>::mins / maxs


@pytest.fixture(scope="module")
def pile150():
    """150x: 900 reads of 5 kb on 30 kb, one pile from the middle (497 windows of 160 strings on average, 179 at most)."""
    d = SynthData(30000, 900, 5000, seed=21)
    ovl, piles = pyoracle.pile_select(d.ovl, d.piles)
    return d, ovl, piles[450:451]


@pytest.fixture(scope="module")
def pile280():
    """250x: 1000 reads of 5 kb on 20 kb, one pile from the middle: windows of up to 310 strings, the ends of the read below 250."""
    d = SynthData(20000, 1000, 5000, seed=21)
    ovl, piles = pyoracle.pile_select(d.ovl, d.piles)
    return d, ovl, piles[500:501]


_oracle = {}


def _oracle_run(name, data, **kw):
    """the oracle's windows and fragments of a (data set, parameters) pair: computed once, shared, never modified"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _oracle:
        d, ovl, sel = data
        p = default_params(**kw)
        O = pyoracle.Oracle(p); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
        fo, bo = O.run(sel, ovl, d.trace, nthreads=4, want_windows=True)
        _oracle[key] = (O.windows(), fo, bo)
    return _oracle[key]


def _emul_run(data, lanes=1, **kw):
    d, ovl, sel = data
    E = emul_lib.Emul(default_params(**kw), lanes=lanes); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fe, be = E.run(sel, ovl, d.trace)
    return E, fe, be


def _deep_count(E, nwindows):
    return nwindows - (sum(E.counts()) + E.count_tier0() + E.count_tier7() + E.count_tier10() + E.count_long())


@pytest.mark.parametrize("lanes,k", [(1, 14), (1, 8), (64, 14)])
def test_150x_pile_finishes_in_the_deep_tier(pile150, lanes, k):
    wo, fo, bo = _oracle_run("pile150", pile150, k=k)
    E, fe, be = _emul_run(pile150, lanes=lanes, k=k)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    ndeep = int((wo["mao"] > MINS).sum())
    assert ndeep == len(wo) and wo["mao"].max() <= MAXS          # every window of this pile is a deep one
    assert E.counts()[3] == 0, E.counts()                         # none in the generic engine
    assert _deep_count(E, len(wo)) == ndeep


def test_mixed_pile_splits_between_deep_tier_and_generic_engine(pile280):
    wo, fo, bo = _oracle_run("pile280", pile280, k=14)
    E, fe, be = _emul_run(pile280, k=14)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    mao = wo["mao"]
    nin = int(((mao > MINS) & (mao <= MAXS)).sum()); nover = int((mao > MAXS).sum())
    assert nin > 0 and nover > 0 and nin + nover == len(wo)
    generic = E.counts()[3]; deep = _deep_count(E, len(wo))
    assert deep > 0 and generic > 0
    assert generic >= nover and deep <= nin and deep + generic == len(wo)       # beyond 250 strings: the generic engine only
    assert deep == nin, (deep, nin)      # at k = 14 these windows find their consensus at filter frequency 2 in a graph tier 3's tables hold


def test_switch_off_restores_the_generic_route(pile150, monkeypatch):
    monkeypatch.setenv("DACC_DEEP_TIER", "0")
    wo, fo, bo = _oracle_run("pile150", pile150, k=14)
    E, fe, be = _emul_run(pile150, k=14)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    assert E.counts()[3] == int((wo["mao"] > MINS).sum()) == len(wo)
    assert _deep_count(E, len(wo)) == 0


def test_windows_of_at_most_96_strings_pass_through_unchanged(monkeypatch):
    """A 50x pile has no window above 96 strings: with the stage in the chain every window finishes where it finished without it."""
    d = SynthData(30000, 300, 5000, seed=7)
    ovl, piles = pyoracle.pile_select(d.ovl, d.piles)
    data = (d, ovl, piles[10:11])
    wo, fo, bo = _oracle_run("pile50", data, k=14)
    assert wo["mao"].max() <= MINS
    E, fe, be = _emul_run(data, k=14)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    on = (E.counts(), E.count_tier10())
    assert _deep_count(E, len(wo)) == 0
    monkeypatch.setenv("DACC_DEEP_TIER", "0")
    E0, f0, b0 = _emul_run(data, k=14)
    assert (E0.counts(), E0.count_tier10()) == on and frags_equal(fo, bo, f0, b0)


def test_high_error_deep_pile_equals_the_oracle():
    """Reads with 30 % errors at 140x, k = 10: some windows find no consensus at filter frequency 2 and go through the passes below it, where
    the graph of a deep window outgrows the tier's node table: the tier hands those on (to the generic engine, tier 3 holds no such window)
    and everything equals the oracle wherever it finishes.  (Measured once, too slow for a test -- 14 minutes in the oracle as in the
    emulation: at 35 % errors 163 of 497 windows need filter frequency 1 and one needs gap filling; the tier finishes 332 windows, hands on
    164, and all of them equal the oracle.)"""
    d = SynthData(30000, 900, 5000, seed=21, erate=0.30)
    ovl, piles = pyoracle.pile_select(d.ovl, d.piles)
    data = (d, ovl, piles[450:451])
    wo, fo, bo = _oracle_run("pile140e30", data, k=10)
    assert (wo["mao"] > MINS).all() and ((wo["status"] == 1) & (wo["filterfreq"] < 2)).any()
    E, fe, be = _emul_run(data, k=10)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    assert _deep_count(E, len(wo)) + E.counts()[3] == len(wo) and _deep_count(E, len(wo)) > 0

"""Shapes of the very-deep-stage tests (tests/test_vdeep_tier.py on the CPU emulation, tests/test_gpu_vdeep_tier.py on the device): seeded data
sets of ONE pile each (aread_range generates only that A read's overlaps), the parameters and the oracle's results -- computed once per process,
shared and never modified.

  M  mixed: 247 windows of 23 ... 291 strings (40 of at most 96, 76 of 97 ... 250, 131 of 251 ... 291); the windows nearest the seams have 247,
     251, 255, 256 and 259 strings: one on each side of the 250 / 251 hand-over and of the 8 bit string id.
  D  deep: 197 windows of 390 ... 792 strings; every true k-mer is seen several hundred times, so the frequency byte and the 40 bit node weight
     of the other tiers are exceeded everywhere.
  X  over the cap: 197 windows of 504 ... 1040 strings, 167 of at most 1000 and 30 of more; windows of 996 and of 1002 strings are both present.

check(name, mao) asserts these properties from the oracle's string counts, so that a changed generator fails loudly instead of testing nothing."""
import pyoracle
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData

MINS, MAXS = 250, 1000      # FastTier<15>::mins / maxs
DEEP_MINS = 96              # FastTier<12>::mins

SHAPES = {
    "M": dict(synth=dict(genome_len=8000, nreads=1200, read_len=2500, seed=21, aread_range=(600, 601))),
    "D": dict(synth=dict(genome_len=6000, nreads=2000, read_len=2000, seed=21, aread_range=(1000, 1001))),
    "X": dict(synth=dict(genome_len=6000, nreads=2480, read_len=2000, seed=21, aread_range=(1240, 1241))),
}

_data = {}
_oracle = {}


def shape(name):
    """(data set, selected overlaps, selected piles) of a shape: its one pile"""
    if name not in _data:
        d = SynthData(**SHAPES[name]["synth"])
        ovl, piles = pyoracle.pile_select(d.ovl, d.piles)
        assert len(piles) == 1
        _data[name] = (d, ovl, piles)
    return _data[name]


def oracle(name, k=14, nthreads=8):
    """(windows, fragments, bases) of the oracle"""
    if (name, k) not in _oracle:
        d, ovl, sel = shape(name)
        O = pyoracle.Oracle(default_params(k=k)); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
        fo, bo = O.run(sel, ovl, d.trace, nthreads=nthreads, want_windows=True)
        _oracle[(name, k)] = (O.windows(), fo, bo)
    return _oracle[(name, k)]


def check(name, wo):
    """the properties of the shape the tests rely on, from the oracle's windows"""
    mao = wo["mao"]; ff = wo["filterfreq"]
    n = lambda m: int(m.sum())
    if name == "M":
        assert len(mao) == 247 and (mao.min(), mao.max()) == (23, 291)
        assert (n(mao <= DEEP_MINS), n((mao > DEEP_MINS) & (mao <= MINS)), n(mao > MINS)) == (40, 76, 131)
        assert {247, 251, 255, 256, 259} <= set(int(v) for v in mao)
        assert (n(ff == 1), n(ff == 2)) == (5, 242)
    elif name == "D":
        assert len(mao) == 197 and (mao.min(), mao.max()) == (390, 792) and (ff == 2).all()
    elif name == "X":
        assert len(mao) == 197 and (mao.min(), mao.max()) == (504, 1040) and (ff == 2).all()
        assert (n(mao <= MAXS), n(mao > MAXS)) == (167, 30)
        assert {996, 1002} <= set(int(v) for v in mao)
    else:
        raise KeyError(name)

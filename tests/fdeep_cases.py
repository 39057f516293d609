"""Shapes of the full-depth stage's tests (tests/test_fdeep_tier.py on the CPU emulation, tests/test_gpu_fdeep_tier.py on the device): seeded data sets of
ONE pile each (aread_range generates only that A read's overlaps), the parameters and the oracle's results -- computed once per process, shared and
never modified.

  Q   of tests/xdeep_cases.py: 37 windows of 2070 ... 3363 strings; with maxalign (-d) = N every window has exactly N strings: -d 2001 is the tier's first.
  R   a pile of 6397 overlaps of which the default pile selection keeps 5000 (-D): 37 windows of 1639 ... 5001 strings, 3 of at most 2000 (1639, 1822,
      1961), 33 of 2001 ... 5000, one of exactly 5001 -- the deepest pile a default run can submit.
  R+  the same data with every overlap kept (pile_select(maxinput=100000)), which no front end submits: with -d 5001 20 windows have exactly 5001 strings
      (the tier's last) and 17 have 2063 ... 5000; with -d 5002 the 20 deepest have 5002 and are handed on.

check(name, wo, maxalign) asserts these properties from the oracle's string counts, so that a changed generator fails loudly instead of testing nothing."""
import pyoracle
import xdeep_cases
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData

MINS, MAXS = 250, 5001      # FastTier<18>::mins / maxs
XDEEP_MAXS = 2000           # FastTier<16>::maxs = FDEEP_MINS

R_SYNTH = dict(genome_len=1200, nreads=16000, read_len=400, min_overlap=150, seed=21, aread_range=(8000, 8001))

_data = {}
_oracle = {}


def shape(name):
    """(data set, selected overlaps, selected piles) of a shape: its one pile"""
    if name == "Q":
        return xdeep_cases.shape("Q")
    if name not in _data:
        if "R" not in _data:
            d = SynthData(**R_SYNTH)
            ovl, piles = pyoracle.pile_select(d.ovl, d.piles)
            assert len(piles) == 1
            _data["R"] = (d, ovl, piles)
        if name == "R+":
            d = _data["R"][0]
            ovl, piles = pyoracle.pile_select(d.ovl, d.piles, maxinput=100000)
            assert len(piles) == 1
            _data["R+"] = (d, ovl, piles)
    return _data[name]


def oracle(name, k=14, maxalign=None, nthreads=8):
    """(windows, fragments, bases) of the oracle"""
    if name == "Q":
        return xdeep_cases.oracle("Q", k=k, maxalign=maxalign, nthreads=nthreads)
    if (name, k, maxalign) not in _oracle:
        d, ovl, sel = shape(name)
        kw = dict(k=k) if maxalign is None else dict(k=k, maxalign=maxalign)
        O = pyoracle.Oracle(default_params(**kw)); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
        fo, bo = O.run(sel, ovl, d.trace, nthreads=nthreads, want_windows=True)
        _oracle[(name, k, maxalign)] = (O.windows(), fo, bo)
    return _oracle[(name, k, maxalign)]


def check(name, wo, maxalign=None):
    """the properties of the shape the tests rely on, from the oracle's windows"""
    mao = wo["mao"]; ff = wo["filterfreq"]; st = wo["status"]
    n = lambda m: int(m.sum())
    assert len(mao) == 37 and (st == 1).all() and (ff == 2).all()
    if name == "Q":
        xdeep_cases.check("Q", wo, maxalign)
        if maxalign is None:
            assert mao.min() > XDEEP_MAXS and mao.max() <= MAXS
    elif name == "R":
        assert maxalign is None
        assert len(shape("R")[0].ovl) == 6397 and len(shape("R")[1]) == 5000
        assert (mao.min(), mao.max()) == (1639, 5001)
        assert sorted(int(v) for v in mao[mao <= XDEEP_MAXS]) == [1639, 1822, 1961]
        assert (n(mao <= XDEEP_MAXS), n((mao > XDEEP_MAXS) & (mao <= 5000)), n(mao == 5001), n(mao > MAXS)) == (3, 33, 1, 0)
    elif name == "R+":
        assert len(shape("R+")[1]) == 6397
        if maxalign == 5001:
            assert n(mao == 5001) == 20 and n(mao < 5001) == 17 and n(mao > 5001) == 0
            assert mao[mao < 5001].min() == 2063 and mao[mao < 5001].max() <= 5000
        elif maxalign == 5002:
            assert n(mao == 5002) == 20 and n(mao > 5002) == 0 and n(mao <= MAXS) == 17
        else:
            raise KeyError(maxalign)
    else:
        raise KeyError(name)

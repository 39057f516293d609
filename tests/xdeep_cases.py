"""Shapes of the deepest-stage tests (tests/test_xdeep_tier.py on the CPU emulation, tests/test_gpu_xdeep_tier.py on the device): seeded data sets of
ONE pile each (aread_range generates only that A read's overlaps), the parameters and the oracle's results -- computed once per process, shared and
never modified.

  P  37 windows of 447 ... 1932 strings from 1931 overlaps: 9 of at most 1000 strings, 28 of 1001 ... 2000, none above.
  Q  37 windows of 2070 ... 3363 strings from 4353 overlaps: with maxalign (-d) = N every window has exactly N strings, which puts a whole pile on
     either side of a seam: -d 1000 (tier 15's last), -d 1001 (tier 16's first), -d 2000 (its last), -d 2001 (handed on).
  X  of tests/vdeep_cases.py: its 30 windows of 1001 ... 1040 strings, 1002 among them.

check(name, wo, maxalign) asserts these properties from the oracle's string counts, so that a changed generator fails loudly instead of testing nothing."""
import pyoracle
import vdeep_cases
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData

MINS, MAXS = 250, 2000      # FastTier<16>::mins / maxs
VDEEP_MAXS = 1000           # FastTier<15>::maxs = XDEEP_MINS

SHAPES = {
    "P": dict(synth=dict(genome_len=1200, nreads=5000, read_len=400, min_overlap=150, seed=21, aread_range=(2500, 2501))),
    "Q": dict(synth=dict(genome_len=1200, nreads=7500, read_len=400, min_overlap=150, seed=21, aread_range=(3750, 3751))),
}

_data = {}
_oracle = {}


def shape(name):
    """(data set, selected overlaps, selected piles) of a shape: its one pile"""
    if name == "X":
        return vdeep_cases.shape("X")
    if name not in _data:
        d = SynthData(**SHAPES[name]["synth"])
        ovl, piles = pyoracle.pile_select(d.ovl, d.piles)
        assert len(piles) == 1
        _data[name] = (d, ovl, piles)
    return _data[name]


def oracle(name, k=14, maxalign=None, nthreads=8):
    """(windows, fragments, bases) of the oracle"""
    if name == "X" and maxalign is None:
        return vdeep_cases.oracle("X", k=k, nthreads=nthreads)
    if (name, k, maxalign) not in _oracle:
        d, ovl, sel = shape(name)
        kw = dict(k=k) if maxalign is None else dict(k=k, maxalign=maxalign)
        O = pyoracle.Oracle(default_params(**kw)); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
        fo, bo = O.run(sel, ovl, d.trace, nthreads=nthreads, want_windows=True)
        _oracle[(name, k, maxalign)] = (O.windows(), fo, bo)
    return _oracle[(name, k, maxalign)]


def check(name, wo, maxalign=None):
    """the properties of the shape the tests rely on, from the oracle's windows"""
    mao = wo["mao"]; ff = wo["filterfreq"]
    n = lambda m: int(m.sum())
    if name == "P":
        assert maxalign is None
        assert len(shape("P")[1]) == 1931
        assert len(mao) == 37 and (mao.min(), mao.max()) == (447, 1932) and (ff == 2).all()
        assert (n(mao <= VDEEP_MAXS), n((mao > VDEEP_MAXS) & (mao <= MAXS)), n(mao > MAXS)) == (9, 28, 0)
    elif name == "Q":
        assert len(shape("Q")[1]) == 4353
        if maxalign is None:
            assert len(mao) == 37 and (mao.min(), mao.max()) == (2070, 3363)
        else:
            assert len(mao) == 37 and (mao == maxalign).all()
    elif name == "X":
        assert maxalign is None
        vdeep_cases.check("X", wo)
        assert n(mao > VDEEP_MAXS) == 30 and mao.max() <= MAXS and 1002 in set(int(v) for v in mao)
    else:
        raise KeyError(name)

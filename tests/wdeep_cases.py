"""Shapes of the wide deep stage's tests (tests/test_wdeep_tier.py on the CPU emulation, tests/test_gpu_wdeep_tier.py on the device): the seeded one-pile
data sets "M", "D" and "X" of tests/vdeep_cases.py run with WIDE parameters (w = 64 ... 127), and the oracle's results -- computed once per process, shared
and never modified.

  shape   data, parameters                       windows   strings per window
  WD      D, k=10, w=100, a=25                   77        390 ... 792
  WD64    D, k=14, w=64, a=16                    122       390 ... 792
  WM      M, k=10, w=96, a=24                    102       23 ... 291: 18 of at most 96, 31 of 97 ... 250, 53 of 251 ... 291
  WM8     M, k=8, w=64, a=16                     154       23 ... 291: 26 / 47 / 81
  S250    D, k=14, w=64, a=32, maxalign=250      62        all exactly 250: tier 14's side of the seam
  S251    D, k=14, w=64, a=32, maxalign=251      62        all exactly 251: the stage's first
  S1000   X, k=14, w=64, a=32, maxalign=1000     62        504 ... 1000, none above: the stage's last
  S1001   X, k=14, w=64, a=32, maxalign=1001     62        504 ... 1001, 9 of exactly 1001, which are handed on
  WX      X, k=10, w=80, a=20                    97        504 ... 1040: 84 of at most 1000, 13 above
  WD8     WD at k=8 (dense graph at w = 100): not part of the table the stage was sized on

Every window has status 1 and filter frequency 2 (WM8 and WD8: not asserted).  check(name, wo) asserts these properties from the oracle's string counts, so
that a changed generator fails loudly instead of testing nothing."""
import pyoracle
import vdeep_cases
from daccord_amd._structs import default_params

MINS, MAXS = 250, 1000      # FastTier<19>::mins / maxs
DEEP_MINS = 96              # the LDS tiers of a wide batch hold up to 96 strings

SHAPES = {
    "WD": ("D", dict(k=10, w=100, a=25)),
    "WD64": ("D", dict(k=14, w=64, a=16)),
    "WM": ("M", dict(k=10, w=96, a=24)),
    "WM8": ("M", dict(k=8, w=64, a=16)),
    "S250": ("D", dict(k=14, w=64, a=32, maxalign=250)),
    "S251": ("D", dict(k=14, w=64, a=32, maxalign=251)),
    "S1000": ("X", dict(k=14, w=64, a=32, maxalign=1000)),
    "S1001": ("X", dict(k=14, w=64, a=32, maxalign=1001)),
    "WX": ("X", dict(k=10, w=80, a=20)),
    "WD8": ("D", dict(k=8, w=100, a=25)),
}
assert set(s[0] for s in SHAPES.values()) <= set(vdeep_cases.SHAPES)

_oracle = {}


def params(name):
    """the parameters of a shape (keyword arguments of default_params)"""
    return dict(SHAPES[name][1])


def shape(name):
    """(data set, selected overlaps, selected piles) of a shape: the one pile of its data set"""
    return vdeep_cases.shape(SHAPES[name][0])


def oracle(name, nthreads=8):
    """(windows, fragments, bases) of the oracle"""
    if name not in _oracle:
        d, ovl, sel = shape(name)
        O = pyoracle.Oracle(default_params(**params(name))); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
        fo, bo = O.run(sel, ovl, d.trace, nthreads=nthreads, want_windows=True)
        _oracle[name] = (O.windows(), fo, bo)
    return _oracle[name]


def ndeep(wo):
    """windows of more than 250 strings: the stage's own"""
    return int((wo["mao"] > MINS).sum())


def nover(wo):
    """windows of more than 1000 strings: what the stage refuses at their string count"""
    return int((wo["mao"] > MAXS).sum())


def check(name, wo):
    """the properties of the shape the tests rely on, from the oracle's windows"""
    mao = wo["mao"]; ff = wo["filterfreq"]; st = wo["status"]
    n = lambda m: int(m.sum())
    split = (n(mao <= DEEP_MINS), n((mao > DEEP_MINS) & (mao <= MINS)), n(mao > MINS))
    if name not in ("WM8", "WD8"):
        assert (st == 1).all() and (ff == 2).all()
    if name in ("WD", "WD8"):
        assert len(mao) == 77 and (mao.min(), mao.max()) == (390, 792)
    elif name == "WD64":
        assert len(mao) == 122 and (mao.min(), mao.max()) == (390, 792)
    elif name == "WM":
        assert len(mao) == 102 and (mao.min(), mao.max()) == (23, 291) and split == (18, 31, 53)
    elif name == "WM8":
        assert len(mao) == 154 and (mao.min(), mao.max()) == (23, 291) and split == (26, 47, 81)
    elif name == "S250":
        assert len(mao) == 62 and (mao == 250).all()
    elif name == "S251":
        assert len(mao) == 62 and (mao == 251).all()
    elif name == "S1000":
        assert len(mao) == 62 and (mao.min(), mao.max()) == (504, 1000)
    elif name == "S1001":
        assert len(mao) == 62 and (mao.min(), mao.max()) == (504, 1001) and n(mao == 1001) == 9
    elif name == "WX":
        assert len(mao) == 97 and (mao.min(), mao.max()) == (504, 1040) and (n(mao <= MAXS), n(mao > MAXS)) == (84, 13)
    else:
        raise KeyError(name)

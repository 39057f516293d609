"""Shapes of the last-stage tests (tests/test_last_tier.py on the CPU emulation, tests/test_gpu_last_tier.py on the device): seeded data sets,
the piles taken from them, the parameters, the environment that forces the route, and the oracle's results -- computed once per process,
shared and never modified.

  A  narrow, forced route: DACC_TIERS=25 leaves the first slot alone, so what it hands on (275 windows of at most 16 strings) is what the last
     stage reads; with the default chain every one of them finishes in an LDS tier (most in tier 6).
  W  wide (w = 64), forced route: DACC_TIERS=2 leaves tier 8 alone, which hands 66 windows on; with the default chain tier 9 finishes all of them.
  H  capacity, default chain: 30 % errors at 50x, k = 8.  Ten windows leave tier 3 on its weight table (8193 forward weight records) and used to
     end in the generic engine, each at filter frequency 1."""
import pyoracle
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData

SHAPES = {
    "A": dict(synth=dict(genome_len=100000, nreads=200, read_len=5000, seed=1), piles=(40, 44), params=dict(k=8), env={"DACC_TIERS": "25"}),
    "W": dict(synth=dict(genome_len=50000, nreads=200, read_len=5000, seed=3), piles=(100, 104), params=dict(k=10, w=64, a=16), env={"DACC_TIERS": "2"}),
    "H": dict(synth=dict(genome_len=30000, nreads=300, read_len=5000, seed=7, erate=0.30), piles=(150, 151), params=dict(k=8), env={}),
}
# the windows of shape H that overflow tier 3's weight table (flags 0x80) and nothing else of the LDS chain holds
H_WINDOWS = (116, 117, 163, 164, 165, 175, 256, 257, 303, 409)
# of those, the ones the device-memory tier 13 finishes (CPU emulation, DACC_LAST_AS_SLOT2=1; the device test asserts the same count)
H_FINISHED = 10

_data = {}
_oracle = {}


def shape(name):
    """(data set, selected overlaps, selected piles) of a shape"""
    if name not in _data:
        S = SHAPES[name]
        d = SynthData(**S["synth"])
        ovl, piles = pyoracle.pile_select(d.ovl, d.piles)
        _data[name] = (d, ovl, piles[S["piles"][0]:S["piles"][1]])
    return _data[name]


def params(name):
    return default_params(**SHAPES[name]["params"])


def oracle(name, nthreads=4):
    """(windows, fragments, bases) of the oracle"""
    if name not in _oracle:
        d, ovl, sel = shape(name)
        O = pyoracle.Oracle(params(name)); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
        fo, bo = O.run(sel, ovl, d.trace, nthreads=nthreads, want_windows=True)
        _oracle[name] = (O.windows(), fo, bo)
    return _oracle[name]

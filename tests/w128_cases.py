"""Shapes of the w = 128 tests (tests/test_w128_tier.py on the CPU emulation, tests/test_gpu_w128_tier.py on the device): batches with a window of 128
bases, whose model table has 129 rows and whose consensus is often longer than 128 symbols.  Seeded data sets, the parameters and the oracle's results --
computed once per process, shared and never modified.

  A   SynthData(60000, 150, 3000, seed=140), the default insertion-rich error mix at erate 0.15, 4 piles, k = 12, w = 128, a = 32: 364 windows, 266
      with a consensus of 106 ... 128 symbols, B strings of more than 128 bases in most windows
  D   seed 141, deletion-rich: erate 0.12, ins / del / sub = 0.2 / 0.7 / 0.1, k = 12: 336 windows with a consensus, 308 of them longer than 128 symbols
  E   seed 141, erate 0.15, thirds, k = 10: 364 windows with a consensus, 169 longer than 128 symbols
  K   A's data, two piles, a k range: klow = 13, khigh = 14, a = 64
  S   seam, tspace = 128 (two byte trace values), w = 128, a = 64: longstr_cases.set_block() gives one interior trace block of four overlaps of the pile
      exactly 128, 129, 255 and 256 B bases; the window on that block's A interval, [128 i, 128 i + 128), has exactly that string

check(name, ...) asserts these properties, so that a changed generator fails loudly instead of testing nothing."""
import pyoracle
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData
from longstr_cases import set_block

LMAX = 255                  # longest string FastTier<20> holds
THIRD = 1.0 / 3.0

SHAPES = {
    "A": dict(synth=dict(genome_len=60000, nreads=150, read_len=3000, seed=140, erate=0.15), npiles=4, par=dict(k=12, w=128, a=32)),
    "D": dict(synth=dict(genome_len=60000, nreads=150, read_len=3000, seed=141, erate=0.12, ins_frac=0.2, del_frac=0.7, sub_frac=0.1), npiles=4, par=dict(k=12, w=128, a=32)),
    "E": dict(synth=dict(genome_len=60000, nreads=150, read_len=3000, seed=141, erate=0.15, ins_frac=THIRD, del_frac=THIRD, sub_frac=THIRD), npiles=4, par=dict(k=10, w=128, a=32)),
    "K": dict(synth=dict(genome_len=60000, nreads=150, read_len=3000, seed=140, erate=0.15), npiles=2, par=dict(klow=13, khigh=14, w=128, a=64)),
    # seam: (A block, B length) per overlap that is changed; the A blocks lie four apart, so no window sees two changed blocks
    "S": dict(synth=dict(genome_len=60000, nreads=150, read_len=3000, seed=130, tspace=128), npiles=1, par=dict(k=10, w=128, a=64, tspace=128),
              seam=[(5, 128), (9, 129), (13, 255), (17, 256)]),
}
NWIN = {"A": 364, "D": 364, "E": 364}
# the oracle's windows with a consensus / with one of more than 128 symbols (premises of the tests)
MIN_OK = {"A": 250}
MIN_LONGCONS = {"D": 250, "E": 100}

_data = {}
_allpiles = {}
_oracle = {}


def shape(name):
    """(data set, selected overlaps, selected piles, trace, bytes per trace value) of a shape"""
    if name not in _data:
        S = SHAPES[name]
        d = SynthData(**S["synth"])
        ovl, piles = pyoracle.pile_select(d.ovl, d.piles)
        tr = d.trace
        if "seam" in S:
            tr, done = set_block(ovl, piles, d.trace, 0, S["seam"], d.tspace)
            assert [(b, l) for _, b, l in done] == S["seam"]
        _data[name] = (d, ovl, piles[:S["npiles"]], tr, d.trace_bytes)
        _allpiles[name] = piles
    return _data[name]


def other_piles(name, n=1):
    """n piles of the shape's data set behind the shape's own (a second batch for the same context)"""
    shape(name)
    k = SHAPES[name]["npiles"]
    return _allpiles[name][k:k + n]


def params(name):
    return default_params(**SHAPES[name]["par"])


def oracle_of(name, sel, nthreads=8):
    """(windows, fragments, bases) of the oracle for piles `sel` of the shape's data set"""
    d, ovl, _, tr, tb = shape(name)
    O = pyoracle.Oracle(params(name)); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
    fo, bo = O.run(sel, ovl, tr, trace_bytes=tb, nthreads=nthreads, want_windows=True)
    return O.windows(), fo, bo


def oracle(name, nthreads=8):
    """(windows, fragments, bases) of the oracle for the shape's own piles"""
    if name not in _oracle:
        _oracle[name] = oracle_of(name, shape(name)[2], nthreads)
    return _oracle[name]


def seam_windows(name="S"):
    """{B length: window of the pile whose A interval is the changed block's} of the seam shape (one pile: the window's index in the batch)"""
    S = SHAPES[name]; ts = S["synth"]["tspace"]; a = S["par"]["a"]
    assert S["par"]["w"] == ts and ts % a == 0
    return {blen: ablock * (ts // a) for ablock, blen in S["seam"]}


def block_lengths(name):
    """B lengths of all trace blocks of the shape's piles"""
    import numpy as np
    d, ovl, sel, tr, tb = shape(name)
    out = []
    for p in sel:
        for z in range(int(p["first_ovl"]), int(p["first_ovl"]) + int(p["novl"])):
            t0 = int(ovl[z]["trace_off"]); nb = int(ovl[z]["tlen"]) // 2
            out += [int(tr[t0 + 2 * i + 1]) for i in range(nb)]
    return np.array(out)


def check(name, wo):
    """the properties of the shape the tests rely on"""
    if name in NWIN:
        assert len(wo) == NWIN[name], len(wo)
    if name in MIN_OK:
        assert int((wo["status"] == 1).sum()) >= MIN_OK[name], int((wo["status"] == 1).sum())
    if name in MIN_LONGCONS:
        n = int(((wo["status"] == 1) & (wo["conslen"] > 128)).sum())
        assert n >= MIN_LONGCONS[name], n
    if name == "S":
        d, ovl, sel, tr, tb = shape(name)
        assert len(sel) == 1 and tb == 2
        sw = seam_windows(name)
        assert all(0 < y < len(wo) - 1 for y in sw.values())
        bl = block_lengths(name)
        assert sorted(int(v) for v in bl[bl >= 255]) == [255, 256] and int((bl == 128).sum()) >= 1 and int((bl == 129).sum()) >= 1
        # the oracle saw at least three strings in each of these windows and found a consensus
        for y in sw.values():
            assert wo["mao"][y] >= 3 and wo["status"][y] == 1, (y, wo["mao"][y], wo["status"][y])

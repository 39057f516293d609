"""Shapes of the long-string-stage tests (tests/test_longstr_tier.py on the CPU emulation, tests/test_gpu_longstr_tier.py on the device): wide
batches (w = 64 ... 127) with B window strings of more than 128 bases, the windows the pre-scan puts on the second stream's list.  Seeded data sets,
the parameters and the oracle's results -- computed once per process, shared and never modified.

  N120  natural long strings: SynthData(60000, 150, 3000, seed=130), three piles, k = 10, w = 120, a = 30: 291 windows, 73 on the pre-scan list
  N127  the same at w = 127, a = 32: 273 windows, 194 on the list
  W64   warped: SynthData(100000, 200, 5000, seed=1) with common.warp_trace (every third overlap gets a block of 115 more B bases), one pile,
        k = 8, w = 64, a = 16: 310 windows, 15 on the list, strings of two to three times the window
  W100  the same at w = 100, a = 25: 197 windows, 20 on the list, some strings of more than 255 bases
  W96   no long string: N120's data at w = 96, a = 24: nothing on the list
  S     seam, tspace = 100, w = 100, a = 50: set_block() gives one interior trace block of three overlaps of the pile exactly 128, 129 and 255 B
        bases; the window on that block's A interval, [100 i, 100 i + 100), has exactly that string
  S2    seam, tspace = 126 (two byte trace values), w = 126, a = 63: blocks of 255 and 256 B bases

check(name, ...) asserts these properties, so that a changed generator fails loudly instead of testing nothing."""
import numpy as np
import pyoracle
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData
from common import warp_trace

LMAX = 255                  # longest string FastTier<17> holds
LSLOT = 128                 # longest string the slots' wide tiers (8, 9, 14) hold

SHAPES = {
    "N120": dict(synth=dict(genome_len=60000, nreads=150, read_len=3000, seed=130), npiles=3, par=dict(k=10, w=120, a=30)),
    "N127": dict(synth=dict(genome_len=60000, nreads=150, read_len=3000, seed=130), npiles=3, par=dict(k=10, w=127, a=32)),
    "W96": dict(synth=dict(genome_len=60000, nreads=150, read_len=3000, seed=130), npiles=3, par=dict(k=10, w=96, a=24)),
    "W64": dict(synth=dict(genome_len=100000, nreads=200, read_len=5000, seed=1), npiles=1, par=dict(k=8, w=64, a=16), warp=[0, 1]),
    "W100": dict(synth=dict(genome_len=100000, nreads=200, read_len=5000, seed=1), npiles=1, par=dict(k=8, w=100, a=25), warp=[0, 1]),
    # seam: (A block, B length) per overlap that is changed; the A blocks lie four apart, so no window sees two changed blocks
    "S": dict(synth=dict(genome_len=60000, nreads=150, read_len=3000, seed=130), npiles=1, par=dict(k=10, w=100, a=50), seam=[(6, 128), (12, 129), (18, 255)]),
    "S2": dict(synth=dict(genome_len=60000, nreads=150, read_len=3000, seed=130, tspace=126), npiles=1, par=dict(k=10, w=126, a=63, tspace=126), seam=[(6, 255), (12, 256)]),
}
# the pre-scan lists of the natural and warped shapes (windows with an active B string of more than 128 bases), measured on the emulation
LISTLEN = {"N120": 73, "N127": 194, "W64": 15, "W100": 20, "W96": 0}
# windows that finish in the stage (emulation: Emul.count_long(); device: dacc_timing.longstr_windows)
FINISHED = {"N120": 73, "N127": 192, "W64": 15, "W100": 20, "W96": 0, "S": 4, "S2": 36}

_data = {}
_allpiles = {}
_oracle = {}


def set_block(ovl, piles, trace, pile_id, targets, tspace):
    """One interior trace block of chosen overlaps of a pile gets an exact B length; the bases come from (or go to) the overlap's other interior
    blocks, as in common.warp_trace, so that the B lengths still sum to bepos - bbpos.  targets: [(A block i, B length)] -- the block on the A
    interval [tspace i, tspace (i+1)); each target takes the first overlap of the pile, not used yet, in which that block is interior with two
    blocks to spare on either side.  Returns (new trace, [(overlap, A block, B length)])."""
    tr = trace.copy(); used = set(); done = []
    f, n = int(piles[pile_id]["first_ovl"]), int(piles[pile_id]["novl"])
    for ablock, blen in targets:
        for z in range(f, f + n):
            o = ovl[z]; nb = int(o["tlen"]) // 2; t0 = int(o["trace_off"])
            tgt = ablock - int(o["abpos"]) // tspace
            if z in used or tgt < 3 or tgt > nb - 4:
                continue
            bl = [int(tr[t0 + 2 * i + 1]) for i in range(nb)]
            need = blen - bl[tgt]      # > 0: taken from the others, < 0: given to them
            for i in list(range(1, tgt)) + list(range(tgt + 1, nb - 1)):
                g = min(bl[i] - 40, need) if need > 0 else max(bl[i] - 120, need)
                if (need > 0 and g > 0) or (need < 0 and g < 0):
                    bl[i] -= g; need -= g
                if need == 0:
                    break
            if need != 0:
                continue
            bl[tgt] = blen
            for i in range(nb):
                tr[t0 + 2 * i + 1] = bl[i]
            used.add(z); done.append((z, ablock, blen))
            break
        else:
            raise AssertionError("no overlap of pile %d has A block %d as an interior block" % (pile_id, ablock))
    return tr, done


def shape(name):
    """(data set, selected overlaps, selected piles, trace, bytes per trace value) of a shape"""
    if name not in _data:
        S = SHAPES[name]
        d = SynthData(**S["synth"])
        ovl, piles = pyoracle.pile_select(d.ovl, d.piles)
        tr = d.trace
        if "warp" in S:
            tr = warp_trace(ovl, piles, d.trace, S["warp"])
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


def oracle(name, nthreads=8):
    """(windows, fragments, bases) of the oracle"""
    if name not in _oracle:
        d, ovl, sel, tr, tb = shape(name)
        O = pyoracle.Oracle(params(name)); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
        fo, bo = O.run(sel, ovl, tr, trace_bytes=tb, nthreads=nthreads, want_windows=True)
        _oracle[name] = (O.windows(), fo, bo)
    return _oracle[name]


def seam_windows(name):
    """{B length: window of the pile whose A interval is the changed block's} of a seam shape (one pile: the window's index in the batch)"""
    S = SHAPES[name]; ts = S["synth"].get("tspace", 100); a = S["par"]["a"]
    assert S["par"]["w"] == ts and ts % a == 0
    return {blen: ablock * (ts // a) for ablock, blen in S["seam"]}


def block_lengths(name):
    """B lengths of all trace blocks of the shape's piles (the strings of the block-aligned windows of a seam shape)"""
    d, ovl, sel, tr, tb = shape(name)
    out = []
    for p in sel:
        for z in range(int(p["first_ovl"]), int(p["first_ovl"]) + int(p["novl"])):
            t0 = int(ovl[z]["trace_off"]); nb = int(ovl[z]["tlen"]) // 2
            out += [int(tr[t0 + 2 * i + 1]) for i in range(nb)]
    return np.array(out)


def check(name, wo):
    """the properties of the shape the tests rely on"""
    nwin = {"N120": 291, "N127": 273, "W64": 310, "W100": 197}
    if name in nwin:
        assert len(wo) == nwin[name], len(wo)
    if name in ("W64", "W100"):
        bl = block_lengths(name)
        assert bl.max() <= 250 and int((bl > 200).sum()) == 4      # the pile's warped blocks: more than twice the trace spacing
    if name in ("S", "S2"):
        d, ovl, sel, tr, tb = shape(name)
        assert len(sel) == 1 and tb == (2 if name == "S2" else 1)
        sw = seam_windows(name)
        assert all(0 < y < len(wo) - 1 for y in sw.values())
        # the oracle saw at least three strings in each of these windows and found a consensus
        for y in sw.values():
            assert wo["mao"][y] >= 3 and wo["status"][y] == 1, (y, wo["mao"][y], wo["status"][y])

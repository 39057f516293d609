"""Shapes of the low-complexity parity tests (tests/test_lowcomplex.py on the CPU, tests/test_gpu_lowcomplex.py on the device): data sets whose
GENOME is made of homopolymer runs and short tandem repeats instead of uniformly random bases, so that most windows contain the same k-mer
more than once -- the stretch loops, nodes with several positions per string and large families of reverse paths with equal (front, baselen)
keys, which a random genome reaches by accident or not at all (a 40 base window of random sequence repeats a k-mer in 0.5 % of the cases at
k = 8, in none at k = 14).

genome(length, seed, mode) fills the genome in consecutive blocks of 20 ... 139 bases from a numpy.random.RandomState (a frozen stream).  A block is
left random, or filled by g[i] = g[i-p] with p = 1 (homopolymer), p = 2 ... 4 or p = 5 ... 14 (tandem repeats; the first p bases of a block
continue the sequence in front of it).  "mixed" draws the four kinds equally, "dense" has no random blocks.

Every case is 150 reads of 3000 bases on 60 kb and its first three piles, except the deep one.  The oracle's result of a case is computed once
per process, shared and never modified.  check(name, windows) asserts the properties the tests rely on with the exact recorded counts, so that
a changed generator fails loudly instead of testing nothing: the share of A windows that repeat a k-mer at the case's k (at least 25 % in
every case), the failed windows, the filter frequencies and the largest string count.

reg1 / reg2 are the regression cases of the sort fallback: the reverse paths of one window of each drive the introsort that the
engines replay to its depth limit (many equal keys), where libstdc++ finishes the range by heapsort; before the generic engine reproduced
that, these windows ended as WS_OVERFLOW with flag 0x400 and their reads were skipped."""
import numpy as np
import pyoracle
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData

MIN_REPEAT_SHARE = 0.25


def genome(length, seed, mode):
    """2-bit codes of a low-complexity genome; mode: "mixed" (a quarter of the blocks random) or "dense" (none)"""
    assert mode in ("mixed", "dense")
    rs = np.random.RandomState(seed)
    g = rs.randint(0, 4, size=length).astype(np.uint8)
    i = 0
    while i < length:
        n = int(rs.randint(20, 140))
        kind = int(rs.randint(0, 4)) if mode == "mixed" else int(rs.randint(1, 4))
        p = 0 if kind == 0 else 1 if kind == 1 else int(rs.randint(2, 5)) if kind == 2 else int(rs.randint(5, 15))
        if p:
            for j in range(max(i, p), min(i + n, length)):
                g[j] = g[j - p]
        i += n
    return g


_SHALLOW = dict(genome_len=60000, nreads=150, read_len=3000)
_DEEP = dict(genome_len=30000, nreads=300, read_len=5000)


def _case(params, mode, gseed, synth=None, npiles=3, seed=1, expect=None, **kw):
    s = dict(_SHALLOW if synth is None else synth); s["seed"] = seed; s.update(kw)
    return dict(params=params, mode=mode, gseed=gseed, synth=s, npiles=npiles, expect=expect)


# expect: (windows, windows that repeat a k-mer at klow, status == 2, filterfreq == 1, filterfreq == 2, largest mao), recorded from the oracle
CASES = {
    "k8_mixed":        _case(dict(k=8), "mixed", 1, expect=(891, 602, 1, 323, 521, 11)),
    "k8_dense":        _case(dict(k=8), "dense", 1, expect=(891, 889, 0, 44, 801, 11)),
    "k14_mixed":       _case(dict(k=14), "mixed", 1, expect=(891, 374, 0, 553, 292, 11)),
    "k14_dense":       _case(dict(k=14), "dense", 1, expect=(891, 678, 0, 287, 558, 11)),
    "k6w32_mixed":     _case(dict(k=6, w=32, a=8), "mixed", 1, expect=(1116, 809, 0, 264, 794, 11)),
    "k6w32_dense":     _case(dict(k=6, w=32, a=8), "dense", 1, expect=(1116, 1116, 0, 15, 1043, 11)),
    "k10w63_mixed":    _case(dict(k=10, w=63, a=16), "mixed", 1, expect=(555, 396, 0, 289, 235, 11)),
    "k10w63_dense":    _case(dict(k=10, w=63, a=16), "dense", 1, expect=(555, 555, 0, 54, 471, 11)),
    # the k loop on near-perfect repeats
    "k8_10_e05_mixed": _case(dict(klow=8, khigh=10), "mixed", 1, erate=0.05, expect=(891, 678, 2, 70, 819, 12)),
    "k8_10_e05_dense": _case(dict(klow=8, khigh=10), "dense", 1, erate=0.05, expect=(891, 891, 3, 53, 835, 12)),
    # failures and gap filling
    "k8_e28_mixed":    _case(dict(k=8), "mixed", 1, erate=0.28, expect=(891, 448, 33, 476, 269, 10)),
    "k8_e28_dense":    _case(dict(k=8), "dense", 1, erate=0.28, expect=(891, 830, 0, 216, 589, 10)),
    # the wide tiers 8 / 9 / 14
    "w100_mixed":      _case(dict(k=8, w=100, a=25), "mixed", 1, expect=(351, 297, 2, 168, 160, 11)),
    "w100_dense":      _case(dict(k=8, w=100, a=25), "dense", 1, expect=(351, 351, 0, 15, 317, 11)),
    # the generic engine alone
    "w128_mixed":      _case(dict(k=12, w=128, a=32), "mixed", 1, expect=(273, 225, 14, 176, 66, 11)),
    "w128_dense":      _case(dict(k=12, w=128, a=32), "dense", 1, expect=(273, 273, 0, 55, 203, 11)),
    # one deep case (50 reads deep on average, up to 63 strings): tiers 4 / 2 / 11 / 12
    "deep_k14":        _case(dict(k=14), "mixed", 1, synth=_DEEP, expect=(1491, 717, 0, 8, 1483, 63)),
    # the sort fallback (one window of each reaches introsort's depth limit)
    "reg1":            _case(dict(k=12, w=128, a=32), "mixed", 2, expect=(273, 220, 17, 143, 97, 11)),
    "reg2":            _case(dict(k=12, w=128, a=32), "mixed", 3, expect=(273, 232, 13, 178, 66, 11)),
    # a forward path of more than 64 stretches in one window: the generic engine's candidate decoder held a path's stretches in a list of 64
    # and gave the window up with flag 0x1000, whatever the scratch size
    "chain":           _case(dict(k=12, w=128, a=32), "mixed", 25, expect=(273, 241, 15, 131, 109, 11)),
}

REGRESSION = ("reg1", "reg2")
_data = {}
_oracle = {}


def params(name):
    return default_params(**CASES[name]["params"])


def shape(name):
    """(data set, selected overlaps, the case's piles)"""
    if name not in _data:
        c = CASES[name]
        d = SynthData(genome=genome(c["synth"]["genome_len"], c["gseed"], c["mode"]), **c["synth"])
        ovl, piles = pyoracle.pile_select(d.ovl, d.piles)
        _data[name] = (d, ovl, piles[:c["npiles"]])
    return _data[name]


def oracle(name, nthreads=8):
    """(windows, fragments, bases) of the oracle"""
    if name not in _oracle:
        d, ovl, sel = shape(name)
        O = pyoracle.Oracle(params(name)); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
        fo, bo = O.run(sel, ovl, d.trace, nthreads=nthreads, want_windows=True)
        _oracle[name] = (O.windows(), fo, bo)
    return _oracle[name]


def _read(d, r):
    n = int(d.rlen[r]); o = int(d.boff[r])
    b = d.bps[o:o + (n + 3) // 4]
    return np.stack([(b >> 6) & 3, (b >> 4) & 3, (b >> 2) & 3, b & 3], axis=1).reshape(-1)[:n]


def repeat_windows(name, wo):
    """number of the oracle's windows whose A interval contains some k-mer (k = the case's klow) twice"""
    d, ovl, sel = shape(name)
    p = params(name); w, a, k = int(p.w), int(p.a), int(p.klow)
    n = 0
    for pi, pile in enumerate(sel):
        seq = _read(d, int(pile["aread"]))
        o = ovl[int(pile["first_ovl"]):int(pile["first_ovl"]) + int(pile["novl"])]
        l = int(o["aepos"].max()) if len(o) else 0
        for y in wo["y"][wo["pile"] == pi]:
            s = int(y) * a if int(y) * a + w <= l else l - w
            win = seq[s:s + w]
            v = np.zeros(w - k + 1, np.int64)
            for j in range(k):
                v = v * 4 + win[j:j + w - k + 1]
            n += len(np.unique(v)) < len(v)
    return n


def measure(name, wo):
    """the premise counts of a case, in the order of CASES[name]["expect"]"""
    ff = wo["filterfreq"]; ok = wo["status"] == 1
    return (len(wo), repeat_windows(name, wo), int((wo["status"] == 2).sum()), int((ok & (ff == 1)).sum()), int((ok & (ff == 2)).sum()), int(wo["mao"].max()))


def check(name, wo):
    """the properties of the case the tests rely on, from the oracle's windows"""
    m = measure(name, wo)
    assert m == tuple(CASES[name]["expect"]), (name, m)
    assert m[1] >= MIN_REPEAT_SHARE * m[0], (name, m)
    assert any(c["expect"][2] > 0 for c in CASES.values())      # at least one case has failed windows

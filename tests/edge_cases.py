"""Parameter edges that dacc_create accepts (include/daccord_hip.h: 3 <= k <= 16, 1 <= w <= 128, any a >= 1, tspace 1 ... 512) and that no
random generator of tests/common.py draws: k = 3, 4, 5, windows shorter than k, a > w, a = 1, trace spacings 8 and 512, reads shorter than a
window, a batch whose piles yield no window at all.  One table for tests/test_edge_params.py (CPU emulation) and tests/test_gpu_edge_params.py
(device): parameters, data recipe, number of piles, and what the oracle alone produced for the case on the CPU -- (windows, windows with
status 1, fragments, bases).  The tests first hold the live oracle to these counts, so that no case silently becomes empty.

Data sets and oracle results are computed once per process, shared and never modified."""
import pyoracle
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData

# recipe "main": two piles of 2 kb reads (tspace of the data = the case's); recipe "short": six piles of reads of L bases
MAIN = dict(genome_len=40000, nreads=80, read_len=2000, seed=3)
SHORT = dict(genome_len=3000, nreads=120, seed=5, min_overlap=20)

# name: (params, ("main", tspace) | ("short", L), piles, (windows, status 1, fragments, bases))
CASES = {
    "k3": (dict(k=3), ("main", 100), 2, (394, 202, 2, 1984)),
    "k4": (dict(k=4), ("main", 100), 2, (394, 202, 2, 1970)),
    "k5": (dict(k=5), ("main", 100), 2, (394, 202, 2, 1973)),
    "k3to6": (dict(klow=3, khigh=6), ("main", 100), 2, (394, 202, 2, 1975)),
    "k3_w8_a2": (dict(k=3, w=8, a=2), ("main", 100), 2, (1994, 1039, 2, 1983)),
    "k4_w6_a1": (dict(k=4, w=6, a=1), ("main", 100), 2, (3990, 2076, 2, 2035)),
    "k8_w8_a4": (dict(k=8, w=8, a=4), ("main", 100), 2, (998, 269, 0, 0)),                  # w = k
    "k8_w10_a3": (dict(k=8, w=10, a=3), ("main", 100), 2, (1330, 692, 2, 2086)),
    "k8_w7_a3": (dict(k=8, w=7, a=3), ("main", 100), 2, (1332, 150, 0, 0)),                 # w < k
    "k3_w1_a1": (dict(k=3, w=1, a=1), ("main", 100), 2, (4000, 2, 0, 0)),
    "k3_w3_a1": (dict(k=3, w=3, a=1), ("main", 100), 2, (3996, 818, 0, 0)),
    "k8_w16_a16": (dict(k=8, w=16, a=16), ("main", 100), 2, (250, 129, 2, 2012)),
    "k8_w23_a7": (dict(k=8, w=23, a=7), ("main", 100), 2, (568, 293, 2, 2017)),
    "k8_w40_a40": (dict(k=8, w=40, a=40), ("main", 100), 2, (100, 50, 2, 1915)),
    "k8_w40_a1": (dict(k=8, w=40, a=1), ("main", 100), 2, (3922, 2014, 2, 2003)),
    "k8_w40_a64": (dict(k=8, w=40, a=64), ("main", 100), 2, (64, 33, 0, 0)),                # a > w
    "minwindowcov0": (dict(k=8, minwindowcov=0), ("main", 100), 2, (394, 342, 2, 3346)),
    "minwindowcov1": (dict(k=8, minwindowcov=1), ("main", 100), 2, (394, 342, 2, 3346)),
    "maxalign1": (dict(k=8, maxalign=1), ("main", 100), 2, (394, 0, 0, 0)),
    "maxalign0": (dict(k=8, maxalign=0), ("main", 100), 2, (394, 0, 0, 0)),
    "maxfilterfreq0": (dict(k=8, maxfilterfreq=0), ("main", 100), 2, (394, 202, 2, 1992)),
    "filterfreq3to5": (dict(k=8, minfilterfreq=3, maxfilterfreq=5), ("main", 100), 2, (394, 0, 0, 0)),
    "eminrate0": (dict(k=8, eminrate=0), ("main", 100), 2, (394, 0, 0, 0)),
    "minlen100000": (dict(k=8, minlen=100000), ("main", 100), 2, (394, 202, 0, 0)),
    "tspace8": (dict(k=8, tspace=8), ("main", 8), 2, (394, 202, 2, 1994)),
    "tspace16": (dict(k=8, tspace=16), ("main", 16), 2, (394, 202, 2, 1991)),
    "tspace33": (dict(k=8, tspace=33), ("main", 33), 2, (394, 202, 2, 1989)),
    "tspace400": (dict(k=8, tspace=400), ("main", 400), 2, (394, 202, 2, 1991)),
    "tspace512": (dict(k=8, tspace=512), ("main", 512), 2, (394, 202, 2, 1991)),
    "L30": (dict(k=8), ("short", 30), 6, (0, 0, 0, 0)),                                     # piles, and nothing to launch
    "L45": (dict(k=8), ("short", 45), 6, (8, 0, 0, 0)),
    "L101": (dict(k=8), ("short", 101), 6, (44, 23, 1, 96)),                                # 101, 250: the last .bps byte of a read is not full
    "L250": (dict(k=8), ("short", 250), 6, (132, 132, 6, 1352)),
}
# the rows the 64-lane emulation runs as well (tests/test_edge_params.py)
LANES64 = ("k3", "k4_w6_a1", "k8_w7_a3", "k8_w40_a64", "tspace512", "L101")

_data = {}
_oracle = {}


def data(name):
    """(data set, selected overlaps, the case's piles)"""
    kind, v = CASES[name][1]
    if (kind, v) not in _data:
        d = SynthData(tspace=v, **MAIN) if kind == "main" else SynthData(read_len=v, **SHORT)
        ovl, piles = pyoracle.pile_select(d.ovl, d.piles, trace_bytes=d.trace_bytes)
        _data[(kind, v)] = (d, ovl, piles)
    d, ovl, piles = _data[(kind, v)]
    return d, ovl, piles[:CASES[name][2]]


def params(name):
    return default_params(**CASES[name][0])


def counts(windows, frags, bases):
    return (len(windows), int((windows["status"] == 1).sum()), len(frags), len(bases))


def oracle(name, nthreads=4):
    """(windows, fragments, bases) of the oracle, held to the recorded counts"""
    if name not in _oracle:
        d, ovl, sel = data(name)
        O = pyoracle.Oracle(params(name)); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
        fo, bo = O.run(sel, ovl, d.trace, trace_bytes=d.trace_bytes, nthreads=nthreads, want_windows=True)
        wo = O.windows()
        assert counts(wo, fo, bo) == CASES[name][3], "the oracle's counts for %s changed: %s, recorded %s" % (name, counts(wo, fo, bo), CASES[name][3])
        _oracle[name] = (wo, fo, bo)
    return _oracle[name]

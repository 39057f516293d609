"""Parity on low-complexity sequence (tests/lowcomplex_cases.py: genomes of homopolymer runs and short tandem repeats, where most windows repeat
a k-mer), on the CPU: the oracle against the reference build (oracle/_ref, recordings in tests/golden/ref_outputs.json), the oracle's own
digests (tests/golden/lowcomplex.json: windows, fragments, bases, FASTA), and the host emulation of the kernels against the oracle, bit for bit.

reg1 / reg2 hold the windows whose reverse paths drive the replayed std::sort to introsort's depth limit: before the generic engine reproduced
libstdc++'s heapsort fallback, the emulation ended them with "window kernel scratch capacity exceeded (flags 0x400)" and the device skipped
their reads.  chain holds a window with a forward path of more than 64 stretches, which the generic engine's candidate decoder gave up with
flags 0x1000.  The device side of the same cases: tests/test_gpu_lowcomplex.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import emul_lib
import lowcomplex_cases as lc
import pyoracle
import pyref
from common import sha, arr_digest, reference_result, windows_equal, frags_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lowcomplex.json")
NAMES = sorted(lc.CASES)
LANES64 = ("k8_mixed", "w100_mixed", "reg1")      # one shallow case, the wide one, one of the regression cases

pyref.build()


def frag_rows(fr):
    return [[int(y["aread"]), int(y["first"]), int(y["last"]), int(y["len"])] for y in fr]


def window_digest(w):
    """status, string count and estimated length of every window; consensus, error rate, filter frequency and k of the finished ones"""
    rows = []
    for x in w:
        r = [int(x["pile"]), int(x["y"]), int(x["status"]), int(x["mao"]), int(x["elength"])]
        if x["status"] == 1:
            r += [int(x["conslen"]), bytes(x["cons"]).hex(), int(x["minrate"]), int(x["filterfreq"]), int(x["k"])]
        rows.append(r)
    return [len(rows), sha(json.dumps(rows))]


def digests(name):
    wo, fo, bo = lc.oracle(name)
    return {"windows": window_digest(wo), "frags": [len(fo), sha(json.dumps(frag_rows(fo)))], "bases": [len(bo), sha(bytes(bo))], "fasta": sha(pyoracle.fasta(fo, bo))}


def test_generator_is_frozen():
    """the genome of a seed never changes (numpy.random.RandomState is a frozen stream), and the two modes are what the module says"""
    gold = json.load(open(GOLD))["genome"]
    for mode in ("mixed", "dense"):
        g = lc.genome(60000, 1, mode)
        assert g.dtype == np.uint8 and g.max() <= 3 and arr_digest(g) == gold[mode]
    # dense: every block repeats with a period of at most 14, so at least the blocks' share behind their first 14 bases does
    g = lc.genome(60000, 1, "dense")
    per = np.zeros(len(g), bool)
    for p in range(1, 15):
        per[p:] |= g[p:] == g[:-p]
    assert per.mean() > 0.99


def test_without_a_genome_the_generator_is_what_it_was():
    """SynthData(genome=its own random genome) returns the bytes of SynthData() (the golden digests of the other tests pin the latter)"""
    from daccord_amd.synth import SynthData
    a = SynthData(60000, 150, 3000, seed=2)
    b = SynthData(60000, 150, 3000, seed=2, genome=a.genome)
    for f in ("bps", "boff", "rlen", "ovl", "trace", "piles", "genome", "truth"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    c = SynthData(60000, 150, 3000, seed=2, genome=lc.genome(60000, 1, "mixed"))
    assert c.bps.tobytes() != a.bps.tobytes() and np.array_equal(c.truth[:, 2], a.truth[:, 2])
    with pytest.raises(ValueError):
        SynthData(60000, 150, 3000, seed=2, genome=a.genome[:-1])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_reference_build(name):
    """every case (k <= 14 throughout): FASTA and fragment list of the oracle against the reference's own headers"""
    d, ovl, sel = lc.shape(name)
    wo, fo, bo = lc.oracle(name); lc.check(name, wo)
    p = lc.params(name)

    def obs():
        R = pyref.Reference(p); R.set_error_profile(*d.error_profile()); R.load_db(d.bps, d.boff, d.rlen)
        fr, br = R.run(sel, ovl, d.trace, nthreads=8)
        return {"fasta": sha(pyoracle.fasta(fr, br)), "frags": frag_rows(fr), "bases": len(br)}
    r = reference_result("lowcomplex/%s" % name, obs, k16=(p.khigh > 12))
    assert len(bo) > 2000 and len(bo) == r["bases"] and frag_rows(fo) == r["frags"] and sha(pyoracle.fasta(fo, bo)) == r["fasta"]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_digests(name):
    gold = json.load(open(GOLD))["cases"]
    assert digests(name) == gold[name]


def _emul(name, lanes):
    d, ovl, sel = lc.shape(name)
    E = emul_lib.Emul(lc.params(name), lanes=lanes); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fe, be = E.run(sel, ovl, d.trace)
    return E, fe, be


@pytest.mark.parametrize("name,lanes", [(n, 1) for n in NAMES] + [(n, 64) for n in LANES64])
def test_emulation_equals_the_oracle(name, lanes):
    wo, fo, bo = lc.oracle(name); lc.check(name, wo)
    E, fe, be = _emul(name, lanes)
    assert windows_equal(wo, E.windows()) == [] and frags_equal(fo, bo, fe, be)
    assert pyoracle.fasta(fe, be) == pyoracle.fasta(fo, bo)
    c = E.counts(); p = lc.params(name)
    if p.w > 100:
        assert c == (0, 0, 0, len(wo))      # the generic engine alone
    else:
        assert c[3] < len(wo)               # the tiers finish some


def test_fuzz_script_with_low_complexity_genomes():
    """two rounds of scripts/fuzz_emul_vs_oracle.py --lowcomplex (random run parameters, mode and genome seed drawn per configuration)"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_emul_vs_oracle.py"), "20261018", "2", "--lowcomplex"], capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and "DONE bad=0" in out.stdout and out.stdout.count("lowcomplex") == 2, out.stdout[-2000:] + out.stderr[-2000:]

"""The consensus -> A alignment behind the window kernels, on the device through the C ABI: a tier leaves a pending record for every narrow
window (w <= 64) it finishes and k_emit (one lane per window, in front of the vote) turns it into the final record; wide windows and the generic
engine write final records themselves, so both kinds lie in one batch.  Per-window results and the FASTA equal the live oracle.
Shapes: a shallow 20x batch (tiers 0 / 7 / 1 / 6) at the default window and at the mask and top-bit edges of the one-word alignment
(w = 64, 63, 24), the high-error shape H of tests/last_tier_cases.py (device-memory tier, consensus lengths far from w), a deep 54x batch
(the tier 4 / 2 chain) and a wide batch (w = 96), where nothing is pending and k_emit leaves every record as it found it.  Run with -m gpu."""
import numpy as np
import pytest
import pyoracle
import last_tier_cases as LC
from daccord_amd import engine
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData
from common import windows_equal, frags_equal

pytestmark = pytest.mark.gpu

# name -> (SynthData arguments, slice of the selected piles)
_SHALLOW = dict(genome_len=3000, nreads=30, read_len=2000, seed=11)                           # 30 reads x 2 kb at 20x
_SETS = {"shallow": (_SHALLOW, (0, 30)),
         # the same data set, ten piles of it: at w = 63, 64 and 96 the oracle takes three times as long per pile as at the default window
         "shallow10": (_SHALLOW, (10, 20)),
         "deep": (dict(genome_len=11111, nreads=120, read_len=5000, seed=4), (58, 61))}        # 54x, three piles from the middle
_synth = {}
_oracle = {}


def _set(name):
    kw, (a, b) = _SETS[name]
    key = tuple(sorted(kw.items()))
    if key not in _synth:
        d = SynthData(**kw)
        _synth[key] = (d,) + tuple(pyoracle.pile_select(d.ovl, d.piles))
    d, ovl, piles = _synth[key]
    return d, ovl, piles[a:b]


def _oracle_run(name, **pkw):
    """(windows, fragments, bases) of the oracle: computed once per (data set, parameters), shared, never modified"""
    key = (name, tuple(sorted(pkw.items())))
    if key not in _oracle:
        d, ovl, sel = _set(name)
        O = pyoracle.Oracle(default_params(**pkw)); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
        fo, bo = O.run(sel, ovl, d.trace, nthreads=16, want_windows=True)
        _oracle[key] = (O.windows(), fo, bo)
    return _oracle[key]


def _device_run(name, **pkw):
    d, ovl, sel = _set(name)
    E = engine.Engine(default_params(**pkw)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(sel, ovl, d.trace)
    return E, fx, bx


def _report(what, E, wx):
    t = E.timing()
    print("defer emit %s: windows %d (%d with a consensus), emit_ms %.3f, vote_ms %.3f, window_ms %.2f, first_tier %d, tier_out %s, last_windows %d, last_out %d" %
          (what, len(wx), int((wx["status"] == 1).sum()), t.emit_ms, t.vote_ms, t.window_ms, t.first_tier, list(t.tier_out), t.last_windows, t.last_out))
    return t


def _same(wo, fo, bo, E, fx, bx):
    wx = E.debug_windows()
    assert windows_equal(wo, wx) == []
    assert frags_equal(fo, bo, fx, bx) and engine.fasta(fx, bx) == pyoracle.fasta(fo, bo)
    return wx


def test_shallow_batch_mixes_pending_and_empty_records_and_reruns():
    wo, fo, bo = _oracle_run("shallow", k=14)
    E, fx, bx = _device_run("shallow", k=14)
    wx = _same(wo, fo, bo, E, fx, bx)
    t = _report("shallow", E, wx)
    # the last workgroup of k_emit is partly filled, and groups of 64 lanes hold both kinds of record
    assert len(wx) % 256 != 0
    st = np.asarray(wo["status"])
    mixed = sum(1 for g in range(0, len(st), 64) if 0 < int((st[g:g + 64] == 1).sum()) < len(st[g:g + 64]))
    assert int((st == 0).sum()) > 0 and mixed > 0
    assert t.emit_ms > 0 and t.emit_ms <= t.vote_ms
    # k_emit over final records changes nothing: two more runs on the resident batch give what the first gave
    for _ in range(2):
        E.rerun(); f2, b2 = E.collect()
        assert frags_equal(fx, bx, f2, b2) and engine.fasta(f2, b2) == engine.fasta(fx, bx)
        assert windows_equal(wo, E.debug_windows()) == []
    E.close()


@pytest.mark.parametrize("name,w,a", [("shallow10", 64, 16), ("shallow10", 63, 10), ("shallow", 24, 10)])
def test_mask_and_top_bit_edges_of_the_one_word_alignment(name, w, a):
    wo, fo, bo = _oracle_run(name, k=14, w=w, a=a)
    E, fx, bx = _device_run(name, k=14, w=w, a=a)
    wx = _same(wo, fo, bo, E, fx, bx)
    _report("w=%d" % w, E, wx)
    assert int((wx["status"] == 1).sum()) > 100
    E.close()


def test_high_error_shape_has_final_and_pending_records(monkeypatch):
    for k in ("DACC_TIERS", "DACC_LAST_TIER", "DACC_LAST_AS_SLOT2"):
        monkeypatch.delenv(k, raising=False)
    d, ovl, sel = LC.shape("H")
    wo, fo, bo = LC.oracle("H", nthreads=8)
    E = engine.Engine(LC.params("H")); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(sel, ovl, d.trace)
    wx = _same(wo, fo, bo, E, fx, bx)
    t = _report("H", E, wx)
    assert t.last_windows + t.last_out > 0                      # windows reach the device-memory tier (and what it hands on, k_window)
    cl = np.asarray(wo["conslen"])[np.asarray(wo["status"]) == 1]
    assert int(cl.min()) <= 40 - 10      # consensus lengths far from w (the oracle's shortest has 23 symbols): the lanes of k_emit do not run in lock step
    E.close()


def test_deep_batch_runs_the_chain_of_deep_piles():
    wo, fo, bo = _oracle_run("deep", k=14)
    E, fx, bx = _device_run("deep", k=14)
    wx = _same(wo, fo, bo, E, fx, bx)
    t = _report("deep", E, wx)
    assert t.first_tier == 4 and int(np.asarray(wo["mao"]).max()) > 40
    E.close()


def test_wide_batch_has_nothing_pending():
    wo, fo, bo = _oracle_run("shallow10", k=14, w=96, a=24)
    E, fx, bx = _device_run("shallow10", k=14, w=96, a=24)
    wx = _same(wo, fo, bo, E, fx, bx)
    _report("w=96", E, wx)
    assert int((wx["status"] == 1).sum()) > 50
    E.rerun(); f2, b2 = E.collect()
    assert frags_equal(fx, bx, f2, b2) and windows_equal(wo, E.debug_windows()) == []
    E.close()

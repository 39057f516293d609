"""Parity on low-complexity sequence on the device (tests/lowcomplex_cases.py: genomes of homopolymer runs and short tandem repeats, where most
windows repeat a k-mer): every case through engine.Engine against the live oracle -- per-window records, fragments, bases and FASTA equal, no
pile dropped and no message, and the same again after rerun() + collect().  The counters of timing() are premises: the slots and stages a case
is meant to reach did run.  reg1 / reg2 (introsort's heapsort fallback in the replayed std::sort) and chain (a forward path of more than 64
stretches) lost reads before the generic engine finished such windows: they assert that no read is skipped.  CPU side: tests/test_lowcomplex.py.
Run with -m gpu."""
import pytest
import pyoracle
import lowcomplex_cases as lc
from daccord_amd import engine
from common import windows_equal, frags_equal

pytestmark = pytest.mark.gpu

# what a case is meant to reach (the 1-lane emulation of the same code says where its windows finish: tests/test_lowcomplex.py)
#   dense   k = 6 / 8: dense graphs, the second slot hands on to the dense-graph tier 10 and the third slot to the last stage
#   slots   the first slot hands on
#   wide    w = 100: the wide tiers 8 / 9 run and hand on
#   deep    a deep batch: first tier 4, no window of more than 96 strings
#   generic w = 128: the generic engine alone
ROUTE = {"k8_mixed": "dense", "k8_dense": "dense", "k6w32_mixed": "dense", "k6w32_dense": "dense",
         "k14_mixed": "slots", "k14_dense": "slots", "k10w63_mixed": "slots", "k10w63_dense": "slots", "k8_10_e05_mixed": "slots", "k8_10_e05_dense": "slots",
         "k8_e28_mixed": "slots", "k8_e28_dense": "slots", "w100_mixed": "wide", "w100_dense": "wide", "deep_k14": "deep",
         "w128_mixed": "generic", "w128_dense": "generic", "reg1": "generic", "reg2": "generic", "chain": "generic"}
assert sorted(ROUTE) == sorted(lc.CASES)


def _run(name):
    d, ovl, sel = lc.shape(name)
    E = engine.Engine(lc.params(name)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(sel, ovl, d.trace)
    return E, fx, bx


def _report(what, t, n):
    print("lowcomplex %s: windows %d, first_tier %d, tier_out %s, tier_ms %s, tier0_in %d, tier0_out %d, tier7_in %d, tier7_out %d, tier10_ran %d, tier10_out %d, long_windows %d, "
          "deep_windows %d, deep_out %d, last_windows %d, last_out %d, last_ms %.3f, window_ms %.2f" %
          (what, n, t.first_tier, list(t.tier_out), [round(x, 3) for x in t.tier_ms], t.tier0_in, t.tier0_out, t.tier7_in, t.tier7_out, t.tier10_ran, t.tier10_out, t.long_windows,
           t.deep_windows, t.deep_out, t.last_windows, t.last_out, t.last_ms, t.window_ms))


def _equal(name, E, fx, bx):
    """everything the device returns equals the oracle, and no pile was dropped"""
    wo, fo, bo = lc.oracle(name)
    bad = windows_equal(wo, E.debug_windows())
    assert bad == [], (len(bad), bad[:5])
    assert frags_equal(fo, bo, fx, bx) and bytes(bx) == bytes(bo)
    assert engine.fasta(fx, bx) == pyoracle.fasta(fo, bo)
    st, msgs = E.pile_status()
    assert len(st) == len(lc.shape(name)[2]) and not st.any() and msgs == [], (st, msgs)      # no read skipped


def _again(name, E):
    wo, fo, bo = lc.oracle(name)
    E.rerun(); f2, b2 = E.collect()
    assert frags_equal(fo, bo, f2, b2) and engine.fasta(f2, b2) == pyoracle.fasta(fo, bo)
    st, msgs = E.pile_status()
    assert not st.any() and msgs == []


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_device_equals_the_oracle(name):
    wo, fo, bo = lc.oracle(name); lc.check(name, wo)
    E, fx, bx = _run(name)
    t = E.timing()
    _report(name, t, len(wo))
    _equal(name, E, fx, bx)
    route = ROUTE[name]
    if route == "generic":
        assert list(t.tier_out) == [0, 0, 0] and t.tier_ms[0] == 0 and t.tier_ms[1] == 0 and t.tier_ms[2] == 0 and t.last_ms == 0 and t.window_ms > 0
    elif route == "wide":
        assert t.tier_ms[1] > 0 and 0 < t.tier_out[1] < len(wo) and t.tier_out[2] > 0
        assert t.last_ms > 0 and t.last_windows + t.last_out == t.tier_out[2]
    elif route == "deep":
        assert t.first_tier == 4 and t.tier_out[0] > 0 and t.tier_out[1] > 0 and (t.deep_windows, t.deep_out) == (0, 0)
    elif route == "dense":
        assert t.first_tier == 1 and t.tier_out[1] > 0 and t.tier10_ran == 1 and t.tier10_ms > 0 and t.tier10_out <= t.tier_out[1]
        assert t.tier_out[2] > 0 and t.last_ms > 0 and t.last_windows + t.last_out == t.tier_out[2]
    else:
        assert t.first_tier == 1 and t.tier_out[0] > 0
    _again(name, E)
    E.close()


def test_generic_engine_on_everything(monkeypatch):
    """DACC_NOFAST=1: failures and gap filling at erate 0.28 through the generic engine alone"""
    monkeypatch.setenv("DACC_NOFAST", "1")
    name = "k8_e28_mixed"
    wo, fo, bo = lc.oracle(name); lc.check(name, wo)
    assert int((wo["status"] == 2).sum()) == 33
    E, fx, bx = _run(name)
    t = E.timing()
    _report(name + " (DACC_NOFAST=1)", t, len(wo))
    _equal(name, E, fx, bx)
    assert list(t.tier_out) == [0, 0, 0] and t.tier_ms[0] == 0 and t.last_ms == 0
    _again(name, E)
    E.close()


def test_without_the_hand_over_slots(monkeypatch):
    """DACC_HAND=0: a tier builds its k-mer instances itself instead of taking the sorted ones of the tier in front"""
    monkeypatch.setenv("DACC_HAND", "0")
    name = "k8_dense"
    wo, fo, bo = lc.oracle(name); lc.check(name, wo)
    E, fx, bx = _run(name)
    t = E.timing()
    _report(name + " (DACC_HAND=0)", t, len(wo))
    _equal(name, E, fx, bx)
    assert t.tier_out[1] > 0
    _again(name, E)
    E.close()

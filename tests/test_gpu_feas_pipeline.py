"""The cases of tests/feas_cases.py through the real kernels (computeStretchFeasLanes with its table word one node ahead and the unit of a
task from a prefix count of unit starts): per-window records, fragments, bases and FASTA of the first pass equal the live oracle, and the
same again after a rerun on the resident batch.  The counters of timing() are premises: between them the cases run in the four shallow
window kernels (tiers 0, 7, 1 and 6) and in the deep chain (first tier 4).  Which situations of the function the cases reach is asserted on
the emulation (tests/test_feas_pipeline.py).  Run with -m gpu."""
import pytest
import pyoracle
import feas_cases as fc
from daccord_amd import engine
from common import windows_equal, frags_equal

pytestmark = pytest.mark.gpu


def _report(name, t, n):
    print("feas pipeline %s: windows %d, first_tier %d, tier_out %s, tier_ms %s, tier0 in / out / ms %d / %d / %.3f, tier7 in / out / ms %d / %d / %.3f, tier10_ran %d, last_windows %d, window_ms %.2f" %
          (name, n, t.first_tier, list(t.tier_out), [round(x, 3) for x in t.tier_ms], t.tier0_in, t.tier0_out, t.tier0_ms, t.tier7_in, t.tier7_out, t.tier7_ms, t.tier10_ran, t.last_windows, t.window_ms))


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_device_equals_the_oracle(name):
    wo, fo, bo = fc.oracle(name)
    d, ovl, sel = fc.shape(name)
    E = engine.Engine(fc.params(name)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(sel, ovl, d.trace)
    t = E.timing()
    _report(name, t, len(wo))
    bad = windows_equal(wo, E.debug_windows())
    assert bad == [], (len(bad), bad[:5])
    assert frags_equal(fo, bo, fx, bx) and bytes(bx) == bytes(bo) and engine.fasta(fx, bx) == pyoracle.fasta(fo, bo)
    st, msgs = E.pile_status()
    assert len(st) == len(sel) and not st.any() and msgs == [], (st, msgs)
    # where the case ran
    if name.startswith("d54"):
        assert t.first_tier == 4 and t.tier_ms[0] > 0 and (t.tier0_in, t.tier7_in) == (0, 0)      # the deep chain, no size classes
    else:
        # size classes of a shallow batch: tier 0, what it leaves to tier 7, what that leaves to tier 1; the second slot is tier 6
        assert t.first_tier == 1
        assert t.tier0_in > 0 and t.tier0_ms > 0 and t.tier7_in > 0 and t.tier7_ms > 0
        assert t.tier7_out > 0 and t.tier_ms[0] > t.tier0_ms + t.tier7_ms      # tier 1 ran on what tier 7 left (tier_ms[0] is the first slot: tiers 0 + 7 + 1)
        assert t.tier_out[0] > 0 and t.tier_ms[1] > 0          # and handed windows on to tier 6
    # the resident batch again (dacc_rerun_resident): the same fragments, the same window records
    E.rerun(); f2, b2 = E.collect()
    assert frags_equal(fo, bo, f2, b2) and engine.fasta(f2, b2) == pyoracle.fasta(fo, bo)
    assert windows_equal(wo, E.debug_windows()) == []
    st, msgs = E.pile_status()
    assert not st.any() and msgs == []
    E.close()

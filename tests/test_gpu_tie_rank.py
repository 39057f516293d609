"""Kept candidates of equal weight on the device (fast_window.hpp, the end of traverse(): lane-parallel rank by heap index, lane 0's two heaps
only where their order can reach the window): two piles of config 2 at the benchmark's k, where the 1-lane emulation sends five windows
through the exact route behind the fast one (tests/test_tie_rank.py), and one 54x pile, whose windows run in the deep tiers -- through the
real kernels with the default and with DACC_TIE_FAST=0 (read in dacc_create).  First pass and rerun equal the live oracle in per-window
records, fragments, bases and FASTA, no pile dropped, no message.  Run with -m gpu."""
import pytest
import pyoracle
import feas_need_cases as fn
import tie_rank_cases as tr
from daccord_amd import engine
from common import windows_equal, frags_equal

pytestmark = pytest.mark.gpu

_oracle = {}


def _input(name):
    """(data, overlaps, piles, parameters, the oracle's windows / fragments / bases), computed once per input"""
    if name not in _oracle:
        if name.startswith("cfg2:"):
            d, ovl, sel, p = tr.shape(name)
            O = pyoracle.Oracle(p); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
            fo, bo = O.run(sel, ovl, d.trace, nthreads=8, want_windows=True)
            _oracle[name] = (d, ovl, sel, p, O.windows(), fo, bo)
        else:
            d, ovl, sel = fn.shape(name)
            _oracle[name] = (d, ovl, sel, fn.params(name)) + tuple(fn.oracle(name))
    return _oracle[name]


@pytest.mark.parametrize("fast", ["1", "0"])
@pytest.mark.parametrize("name", ["cfg2:3001:2", "d54_k14"])
def test_first_pass_and_rerun_equal_the_oracle(name, fast, monkeypatch):
    d, ovl, sel, p, wo, fo, bo = _input(name)
    monkeypatch.setenv("DACC_TIE_FAST", fast)
    E = engine.Engine(p); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(sel, ovl, d.trace, trace_bytes=getattr(d, "trace_bytes", 1))
    t = E.timing()
    print("tie rank %s (DACC_TIE_FAST=%s): windows %d, first_tier %d, tier_out %s, tier0 in / out %d / %d, deep_windows %d, window_ms %.2f" %
          (name, fast, len(wo), t.first_tier, list(t.tier_out), t.tier0_in, t.tier0_out, t.deep_windows, t.window_ms))
    bad = windows_equal(wo, E.debug_windows())
    assert bad == [], (len(bad), bad[:5])
    assert frags_equal(fo, bo, fx, bx) and bytes(bx) == bytes(bo) and engine.fasta(fx, bx) == pyoracle.fasta(fo, bo)
    assert t.tier_ms[0] > 0 or t.tier_ms[1] > 0      # the window tiers ran, not the generic engine alone
    E.rerun(); f2, b2 = E.collect()
    assert windows_equal(wo, E.debug_windows()) == []
    assert frags_equal(fo, bo, f2, b2) and bytes(b2) == bytes(bo) and engine.fasta(f2, b2) == pyoracle.fasta(fo, bo)
    st, msgs = E.pile_status()
    assert len(st) == len(sel) and not st.any() and msgs == [], (st, msgs)
    E.close()

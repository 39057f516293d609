"""The accepted parameter edges of tests/edge_cases.py through the real kernels: k = 3, 4, 5, windows shorter than k, a > w, a = 1 (4000
windows per 2 kb read), trace spacings 8 (five times the usual number of trace blocks) and 512 (k_trace_wide<8>), reads shorter than a
window, a batch with piles and no window.  Per-window records and fragments equal the oracle's bit for bit, and the resident re-run
(a zero-length window list included) collects the same fragments again.  Every call must return DACC_OK: a failure carries
dacc_last_error and is a finding to diagnose from that message."""
import pytest
from daccord_amd import engine
import edge_cases as EC
from common import windows_equal, frags_equal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(EC.CASES))
def test_edge_on_the_device(name):
    d, ovl, sel = EC.data(name)
    wo, fo, bo = EC.oracle(name, nthreads=8)
    assert EC.params(name).w <= 79                       # dacc_window_result.cons holds the first 79 bases
    E = engine.Engine(EC.params(name)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(sel, ovl, d.trace, trace_bytes=d.trace_bytes)          # (a non-zero return raises DaccError with dacc_last_error)
    wx = E.debug_windows()
    status, msgs = E.pile_status()
    assert (status == 0).all() and msgs == [], (status, msgs)
    assert len(wx) == EC.CASES[name][3][0]
    bad = windows_equal(wo, wx)
    assert bad == [], (len(bad), bad[:5])
    assert frags_equal(fo, bo, fx, bx)
    assert EC.counts(wx, fx, bx) == EC.CASES[name][3]
    E.rerun(); f2, b2 = E.collect()
    assert frags_equal(fo, bo, f2, b2)
    E.close()

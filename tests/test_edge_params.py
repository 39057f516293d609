"""The accepted parameter edges of tests/edge_cases.py on the CPU emulation of the kernel headers: every row on the 1-lane wavefront, a
few on the 64-lane one, bit for bit against the oracle -- per-window records and fragments.  (tests/test_gpu_edge_params.py runs the
same table through the launches, grids, LDS layouts and trace kernels of the device.)"""
import pytest
import emul_lib
import edge_cases as EC
from common import windows_equal, frags_equal


def _run(name, lanes):
    d, ovl, sel = EC.data(name)
    wo, fo, bo = EC.oracle(name)
    E = emul_lib.Emul(EC.params(name), lanes=lanes); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fe, be = E.run(sel, ovl, d.trace, trace_bytes=d.trace_bytes)
    we = E.windows()
    assert len(we) == EC.CASES[name][3][0]
    bad = windows_equal(wo, we)
    assert bad == [], (len(bad), bad[:5])
    assert frags_equal(fo, bo, fe, be)
    assert EC.counts(we, fe, be) == EC.CASES[name][3]


@pytest.mark.parametrize("name", list(EC.CASES))
def test_edge_one_lane(name):
    _run(name, 1)


@pytest.mark.parametrize("name", EC.LANES64)
def test_edge_64_lanes(name):
    _run(name, 64)

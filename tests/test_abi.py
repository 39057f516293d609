"""The drop-in boundary without a GPU: the library loads, exports every symbol include/daccord_hip.h
declares, refuses to run without a HIP device (no CPU fallback), and its host-side pile selection equals
the oracle's restatement of daccord.cpp:2120-2288."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import pyoracle
from daccord_amd import engine
from daccord_amd._structs import default_params, DaccOverlap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_match_header():
    hdr = open(os.path.join(ROOT, "include", "daccord_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(dacc_[a-z_]+)\s*\(", hdr)))
    L = engine.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert set(engine.EXPORTS) <= set(declared)


def test_io_exports_match_header():
    """include/daccord_io.h: every entry point is exported by the host-only library and by the HIP library."""
    from daccord_amd import io as dio
    hdr = open(os.path.join(ROOT, "include", "daccord_io.h")).read()
    declared = sorted(set(re.findall(r"\b(dacc_(?:db|las)_[a-z_]+)\s*\(", hdr)))
    assert len(declared) >= 10
    for L in (dio.lib(), engine.lib()):
        for name in declared:
            assert hasattr(L, name), name


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(engine.DaccError) as e:
        engine.Engine(default_params())
    assert e.value.code == -2                              # DACC_ENODEV


def test_bad_params_rejected():
    for kw in (dict(k=2), dict(k=17), dict(klow=9, khigh=8), dict(w=0), dict(w=129), dict(tspace=0), dict(tspace=513), dict(tspace=1000)):
        h = C.c_void_p()
        rc = engine.lib().dacc_create(C.byref(h), C.byref(default_params(**kw)))
        assert rc == -1, kw


def _plan_only(p, d, ovl, piles):
    L = engine.lib()
    L.dacc_plan_only.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int,
                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    rlen = np.ascontiguousarray(d.rlen, np.uint32); piles = np.ascontiguousarray(piles); ovl = np.ascontiguousarray(ovl); tr = np.ascontiguousarray(d.trace)
    nw = C.c_uint64(12345); nb = C.c_uint64(12345)
    rc = L.dacc_plan_only(C.byref(p), rlen.ctypes.data, len(rlen), piles.ctypes.data if len(piles) else None, len(piles), ovl.ctypes.data, len(ovl),
                          tr.ctypes.data, tr.nbytes // d.trace_bytes, d.trace_bytes, C.byref(nw), C.byref(nb))
    return rc, nw.value, nb.value


def test_trace_spacing_contract_of_the_planner():
    """include/daccord_hip.h: tspace 1 ... 512.  The planner (batch_plan.hpp, before anything is uploaded) refuses a larger spacing with
    DACC_ENOTSUP and plans 512 and 1; no device is involved, and no test submits a spacing above 512 to one."""
    import edge_cases as EC
    d, ovl, piles = EC.data("tspace512")
    assert d.trace_bytes == 2
    rc, nw, nb = _plan_only(default_params(k=8, tspace=512), d, ovl, piles)
    assert rc == 0 and nw == EC.CASES["tspace512"][3][0] and nb > 0
    for ts in (513, 1000):
        rc, nw, nb = _plan_only(default_params(k=8, tspace=ts), d, ovl, piles)
        assert rc == -6 and nw == 0 and nb == 0, (ts, rc, nw, nb)          # DACC_ENOTSUP
    # spacing 1: one trace block per base
    from daccord_amd.synth import SynthData
    d1 = SynthData(3000, 30, 300, seed=5, min_overlap=100, tspace=1)
    o1, p1 = pyoracle.pile_select(d1.ovl, d1.piles)
    assert len(o1) > 0 and (o1["tlen"] == 2 * (o1["aepos"] - o1["abpos"])).all()
    rc, nw, nb = _plan_only(default_params(k=8, tspace=1), d1, o1, p1[:4])
    assert rc == 0 and nw > 0 and nb == int(o1["tlen"][:int(p1[3]["first_ovl"] + p1[3]["novl"])].sum()) // 2, (rc, nw, nb)
    # and an empty batch
    assert _plan_only(default_params(k=8, tspace=1), d1, o1, p1[:0])[0] == 0
    assert _plan_only(default_params(k=8, tspace=513), d1, o1, p1[:0])[0] == -6


def test_pile_select_matches_oracle(small_data):
    d, _, _ = small_data
    for maxinput in (5000, 7, 1):
        a, pa = engine.pile_select(d.ovl, d.piles[:20], maxinput=maxinput)
        b, pb = pyoracle.pile_select(d.ovl, d.piles[:20], maxinput=maxinput)
        assert a.tobytes() == b.tobytes() and pa.tobytes() == pb.tobytes()
    # a pile larger than one 64 KiB input block (block-wise copy order, daccord.cpp:2199-2262)
    rng = np.random.default_rng(3)
    big = np.zeros(3000, dtype=np.dtype(DaccOverlap))
    big["abpos"] = rng.integers(0, 50, 3000); big["aepos"] = big["abpos"] + 1000 + rng.integers(0, 100, 3000)
    big["diffs"] = rng.integers(0, 300, 3000); big["tlen"] = 22; big["bread"] = np.arange(3000)
    from daccord_amd._structs import DaccPile
    piles = np.zeros(1, dtype=np.dtype(DaccPile)); piles[0]["novl"] = 3000
    for maxinput in (5000, 100):
        a, pa = engine.pile_select(big, piles, maxinput=maxinput)
        b, pb = pyoracle.pile_select(big, piles, maxinput=maxinput)
        assert a.tobytes() == b.tobytes()
        assert (np.diff(a["abpos"]) >= 0).all()

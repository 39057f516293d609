"""The filter of computeStretchFeasLanes: only the (stretch, direction, start position) triples that the enumerations of a traversal can read
get a task -- forward units from the shortest distance of their first node to a first k-mer candidate up to H = (lmax+1)/2, reverse units
whole, where a path of base length below H can reach their last node (fast_window.hpp: feasDistances, computeStretchFeasLanes).

Every case of tests/feas_need_cases.py runs on the host emulation of the kernels with the filter and without it (DACC_FEAS_NEED=0), with one
lane and, two of them, with 64: the windows, fragments, bases and FASTA of both runs equal the live oracle and each other.  The audit aid of
the emulation (DACC_EMUL_FEASNEED) remembers per traversal what the filter left out and counts every sfFind / csfFind of a left-out position and
every linkOk on a left-out reverse unit: none may happen, in the cases and in two piles of config 2 (the benchmark's data).  Its other columns
are premises -- the filter did leave tasks out, and the cases went through the situations they are there for -- so that no test passes by
filtering nothing or by never reaching its case.  The runs of a wavefront width share one process; the tests of this file share the runs.
The device side: tests/test_gpu_feas_need.py."""
import json
import os
import subprocess
import sys

import pytest

import emul_lib
import feas_need_cases as fn

HERE = os.path.dirname(os.path.abspath(__file__))
ONE_LANE = sorted(fn.CASES)

emul_lib.build()
_runs = {}


def _script(tmp, tag, script, args):
    audit = os.path.join(str(tmp), tag + ".audit")
    out = subprocess.run([sys.executable, os.path.join(HERE, script)] + [a.replace("@AUDIT@", audit) for a in args], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]


def runs(lanes, tmp):
    """case -> result line of its two runs at this wavefront width"""
    if lanes not in _runs:
        names = ONE_LANE if lanes == 1 else list(fn.LANES64)
        res = _script(tmp, "cases%d" % lanes, "feas_need_cases.py", [str(lanes), "@AUDIT@"] + names)
        assert [r["case"] for r in res] == names
        _runs[lanes] = {r["case"]: r for r in res}
    return _runs[lanes]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("feasneed")


RUNS = [(n, 1) for n in ONE_LANE] + [(n, 64) for n in fn.LANES64]


@pytest.mark.parametrize("name,lanes", RUNS)
def test_filtered_and_unfiltered_equal_the_oracle(name, lanes, tmp):
    r = runs(lanes, tmp)[name]
    for need in ("1", "0"):
        assert r["bad_windows_" + need] == 0 and r["equal_" + need], (need, r)
        assert r["fast_windows_" + need] > 0 and r["audit_" + need]["traversals"] > 0      # the tiers finish windows, and the traversals were audited
    assert r["on_equals_off"]


@pytest.mark.parametrize("name,lanes", RUNS)
def test_nothing_left_out_is_ever_read(name, lanes, tmp):
    a = runs(lanes, tmp)[name]["audit_1"]
    print("feas need %s (%d lanes): %s" % (name, lanes, a))
    assert (a["probes_f"], a["probes_r"], a["links_r"]) == (0, 0, 0)
    # ... and the filter is on: fewer units with tasks, fewer tasks, than without it
    assert a["tasks_kept"] < a["tasks_all"] and a["units_kept"] < a["units_all"]


@pytest.mark.parametrize("name,lanes", RUNS)
def test_the_switch_restores_the_full_computation(name, lanes, tmp):
    r = runs(lanes, tmp)[name]
    a1, a0 = r["audit_1"], r["audit_0"]
    assert a0["tasks_kept"] == a0["tasks_all"] and a0["units_kept"] == a0["units_all"] and a0["relax_passes"] == 0
    assert (a0["probes_f"], a0["probes_r"], a0["links_r"]) == (0, 0, 0)
    # the same traversals either way (which tier finishes a window does not depend on the filter), fewer weight records with it
    assert a1["traversals"] == a0["traversals"]
    assert a1["rec_f"] + a1["rec_r"] < a0["rec_f"] + a0["rec_r"]


def test_64_lanes_filter_what_one_lane_filters(tmp):
    for name in fn.LANES64:
        a1, a64 = runs(1, tmp)[name]["audit_1"], runs(64, tmp)[name]["audit_1"]
        b1 = {n: a1[n] for n in fn.AUDIT if n != "relax_passes"}      # (lanes that relax the same node in one step may need another pass)
        b64 = {n: a64[n] for n in fn.AUDIT if n != "relax_passes"}
        assert b1 == b64, (name, b1, b64)


def test_cases_reach_their_situations(tmp):
    R = runs(1, tmp)
    A = {n: R[n]["audit_1"] for n in ONE_LANE}
    # candidates strictly inside a stretch, and a first and a last one inside the same stretch
    assert A["s20_k14"]["first_inside"] > 0 and A["s20_k14"]["last_inside"] > 0
    assert A["lc_k14"]["middle_pieces"] > 0
    # the distances need more than the pass that finds nothing to change: paths of several stretches, loops
    for n in ("s20_k8", "lc_k8", "lc_k14"):
        assert A[n]["relax_passes"] > 2 * A[n]["traversals"], (n, A[n])
    # H <= k in most traversals of the short windows (lmax follows the estimated length of a window: a few reach 2k and more), in none at
    # k = 8 and w = 40
    assert 2 * A["w24_k14"]["h_le_k"] > A["w24_k14"]["traversals"] and A["s20_k8"]["h_le_k"] == 0
    assert R["ff0"]["ff0"] > 0      # windows decided at filter frequency 0
    assert R["w96_k8"]["wide"] and R["w96_k8"]["fast_windows_1"] > 0
    assert R["d54_k14"]["fast_windows_1"] > 0


def test_two_piles_of_config_2(tmp):
    """the first two piles of the benchmark's data set at its k: nothing left out is read, outputs with and without the filter are equal"""
    res = _script(tmp, "cfg2", "feas_need_cfg2.py", ["@AUDIT@", "2"])
    assert len(res) == 1
    r = res[0]
    print("feas need cfg2: %s" % r)
    a = r["audit_1"]
    assert r["on_equals_off"] and r["windows"] > 1000
    assert (a["probes_f"], a["probes_r"], a["links_r"]) == (0, 0, 0)
    assert a["tasks_kept"] < a["tasks_all"] and a["units_kept"] < a["units_all"]

"""computeStretchFeasLanes (stretch feasibility, one lane per (stretch, direction, start position)) with its table word one node ahead and
the unit of a task from a prefix count of unit starts instead of a binary search: bit parity on the host emulation of the kernels, with one lane
and with 64, against the live oracle, and a record-level pin against the traces of the code before the change.

Every case (tests/feas_cases.py) runs once per wavefront width in a process of its own, because the emulation opens its trace files once per
process; the runs are shared by the tests of this file.  The emulation's counters (DACC_EMUL_FEASCASES: one line per traversal) say which
situations the cases went through; test_cases_reach_every_situation asserts each of them, so that no test passes by never reaching its case.
The rounds of 64 tasks exist only on the 64-lane wavefront: the situations that concern them are asserted on the 64-lane runs.

Three situations one could list do not exist in this code, whatever the input; the counters pin that too:
  * a stretch of ONE node: a stretch holds its first and its last node (poolKey reads its second link), the shortest has two;
  * a position P + j AT or BEHIND the table's clamp row: a unit's start positions are the intersection of its nodes' support ranges
    shifted by j, so P + j stays inside node j's range, below nrows; only the table word fetched one node AHEAD, behind the last node of a
    stretch, reaches the clamp row (P + len = nrows) -- that one is counted (at_clamp) and must occur;
  * a traversal without tasks: every stretch was walked from k-mer instances of the window, whose positions are in all of its ranges.
The device side of the same cases: tests/test_gpu_feas_pipeline.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import emul_lib
import feas_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "feas_pipeline_trav.txt")
ONE_LANE = sorted(fc.CASES)
RUNS = [(n, 1) for n in ONE_LANE] + [(n, 64) for n in fc.LANES64]

emul_lib.build()
_runs = {}


def run(name, lanes, tmp):
    """(result line of the run, counters [traversals x columns], summary lines of the traversal trace)"""
    if (name, lanes) not in _runs:
        prefix = os.path.join(str(tmp), "%s_%d" % (name, lanes))
        out = subprocess.run([sys.executable, os.path.join(HERE, "feas_cases.py"), name, str(lanes), prefix], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        cases = np.loadtxt(prefix + ".cases", dtype=np.uint64, ndmin=2)
        assert cases.shape[1] == len(fc.COLUMNS)
        # the per-traversal summary lines (tier, strings, graph sizes, nwF, nwR, candidates); "R" / "T" lines are per enumeration
        trav = [l for l in open(prefix + ".trav").read().splitlines() if l and l[0] not in "RT"]
        _runs[(name, lanes)] = (res, cases, trav)
    return _runs[(name, lanes)]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("feas")


def col(cases, name):
    return cases[:, fc.COLUMNS.index(name)]


@pytest.mark.parametrize("name,lanes", RUNS)
def test_emulation_equals_the_oracle(name, lanes, tmp):
    res, cases, trav = run(name, lanes, tmp)
    assert res["bad_windows"] == 0 and res["frags_equal"] and res["fasta_equal"]
    assert res["counts"][3] < res["windows"] and len(cases) > 0      # the tiers finish windows, and the traversals were traced


@pytest.mark.parametrize("name", fc.LANES64)
def test_64_lanes_append_what_one_lane_appends(name, tmp):
    """per traversal: the same units, tasks, nodes walked, failures and numbers of forward / reverse weight records (nwF, nwR)"""
    _, c1, t1 = run(name, 1, tmp)
    _, c64, t64 = run(name, 64, tmp)
    assert np.array_equal(c1, c64) and t1 == t64


@pytest.mark.parametrize("lanes", [1, 64])
def test_record_level_pin(lanes, tmp):
    """tests/golden/feas_pipeline_trav.txt: the summary line of every traversal of case "pin" from the emulation of the code before the
    change (DACC_EMUL_TRAV: tier, strings, graph sizes, nwF, nwR, number of candidates), line for line"""
    _, _, trav = run("pin", lanes, tmp)
    gold = open(GOLD).read().splitlines()
    assert len(gold) > 300 and trav == gold


def test_cases_reach_every_situation(tmp):
    one = np.concatenate([run(n, 1, tmp)[1] for n in ONE_LANE])
    w64 = np.concatenate([run(n, 64, tmp)[1] for n in fc.LANES64])
    for c, what in ((one, "1 lane"), (w64, "64 lanes")):
        lens = int(np.bitwise_or.reduce(col(c, "lenmask")))
        tot = {n: int(col(c, n).sum()) for n in fc.COLUMNS}
        print("feas situations (%s): traversals %d, tasks %d, rounds %d, nodes %d, %s, lengths 0x%x, longest %d, units up to %d" %
              (what, len(c), tot["ntask"], tot["rounds"], tot["nodes"], {n: tot[n] for n in fc.COLUMNS[4:10] + fc.COLUMNS[13:19]}, lens, int(col(c, "maxlen").max()), int(col(c, "nu").max())))
        # pipeline prologue and epilogue: stretches of 2, 3, 4 and 5 nodes, and long ones (a window of 40 bases at k = 8 has 33 k-mers)
        assert all(lens >> n & 1 for n in (2, 3, 4, 5)) and int(col(c, "maxlen").max()) >= 30
        assert not lens & 3                                              # no stretch of one node (see the module's text)
        # the table word fetched ahead reaches the clamp row; P + j itself never does
        assert tot["at_clamp"] > 0 and tot["past_clamp"] == 0
        assert tot["multi"] > 0                                          # nodes with several instances
        assert tot["fail0"] > 0 and tot["fail1"] > 0 and tot["faillast"] > 0      # infeasible at node 0, at node 1, at the last node (of three or more)
        assert int((col(c, "nu") > 64).sum()) > 0                        # the unit order spans chunks of 64
        assert tot["empty_first"] > 0 and tot["empty_mid"] > 0 and tot["empty_last"] > 0      # units without a task at the start, inside and at the end of the order
        # a unit whose first task is the first / the last task of a round of 64, a unit that spans two rounds
        assert tot["start_at_round"] > 0 and tot["start_at_round_end"] > 0 and tot["spans_rounds"] > 0
        assert int((col(c, "ntask") < 64).sum()) > 0                     # a traversal of less than one round
        assert int((col(c, "ntask") == 0).sum()) == 0                    # none without tasks (see the module's text)
    # every tier class of the cases: shallow 28 / 28 / 32 / 40 strings (tiers 0, 7, 1, 6), dense and deep 64 / 96
    assert {28, 32, 40, 96} <= set(int(x) for x in col(one, "tier"))

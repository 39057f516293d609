"""Kept candidates of equal weight (fast_window.hpp, the end of traverse()): the lane-parallel rank orders them by their index in the candidate
heap, and lane 0's two heaps -- whose mechanics order them in the reference -- run only when that order can reach the window: a candidate
ties entry 0 of the final sort in error sum and weight and spells another string.  Then decode, errors and sort run once more from the
heaps' order, so the result is the reference's in every window.

The inputs run on the host emulation (tests/tie_rank_cases.py) with the default and with DACC_TIE_FAST=0 (every tie takes the heaps, as
before the change); both equal the live oracle and each other.  The emulation counts the windows that took the exact route after the fast
one (column 32 of the DACC_EMUL_STATS line): more than none, so the route is exercised, and at most 1 % of the windows, so the ambiguity
test is no wider than it has to be (24 piles of config 2 from pile 3000, the benchmark's data: 159 of 23 928 windows, 0.66 %; 35 % have a
tie; ranking by heap index alone, without the exact route, would change the consensus of 85 windows, 0.36 %).  Per-window status, filter
frequency, k and consensus length, the tier counts and the overflow flags -- every over() call of every tier in order, the flags each slot
hands on with, the generic engine's (window, flags) list -- are those of the commit before the change (tests/golden/tie_rank_state.json,
recorded from its emulation library by tests/tie_rank_cases.py --record).  The device side: tests/test_gpu_tie_rank.py."""
import json
import os
import subprocess
import sys

import pytest

import emul_lib
import tie_rank_cases as tr

HERE = os.path.dirname(os.path.abspath(__file__))
CFG2 = "cfg2:3000:24"          # piles 3000 ... 3023 of config 2 at k = 14
CFG2_64 = "cfg2:3001:2"        # piles 3001 ... 3002: five windows of the 1-lane run take the exact route (3001 y = 161, 3002 y = 118 / 295 / 412 / 898)
STATE_CASES = (CFG2, "lc_k8", "w24_k14")

emul_lib.build()
_runs = {}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("tierank")


def runs(lanes, tmp):
    if lanes not in _runs:
        names = list(STATE_CASES) if lanes == 1 else [CFG2_64]
        out = subprocess.run([sys.executable, os.path.join(HERE, "tie_rank_cases.py"), str(lanes), os.path.join(str(tmp), "stats%d" % lanes)] + names,
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        res = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
        assert [r["case"] for r in res] == names
        _runs[lanes] = {r["case"]: r for r in res}
        for r in res:
            print("tie rank (%d lanes): %s" % (lanes, r))
    return _runs[lanes]


def test_config_2_equals_the_oracle_and_few_windows_take_the_exact_route(tmp):
    r = runs(1, tmp)[CFG2]
    assert r["windows"] > 20000
    assert r["bad_windows_1"] == 0 and r["equal_1"], r
    assert r["exact_1"] > 0, r                          # the exact route runs
    assert 100 * r["exact_1"] <= r["windows"], r        # ... in at most 1 % of the windows
    assert r["ties_1"] > 10 * r["exact_1"], r           # equal weights are common, decisive ones are not


def test_the_switch_restores_the_heaps_for_every_tie(tmp):
    r = runs(1, tmp)[CFG2]
    assert r["bad_windows_0"] == 0 and r["equal_0"], r
    assert r["on_equals_off"], r
    assert r["exact_0"] == 0 and r["ties_0"] == r["ties_1"], r


def test_64_lanes_on_two_piles(tmp):
    r = runs(64, tmp)[CFG2_64]
    assert r["bad_windows_1"] == 0 and r["equal_1"] and r["bad_windows_0"] == 0 and r["equal_0"] and r["on_equals_off"], r
    assert r["exact_1"] >= 5 and r["exact_0"] == 0, r


@pytest.mark.parametrize("name", STATE_CASES)
def test_status_flags_and_tiers_are_the_parents(name, tmp):
    r = runs(1, tmp)[name]
    assert r["bad_windows_1"] == 0 and r["equal_1"] and r["on_equals_off"], r
    gold = json.load(open(tr.GOLDEN))[name]
    got = r["state"]
    print("tie rank state %s: %d over() calls %s, handed on %s, generic %d windows" % (name, got["over_events"], got["over_bits"], got["handed_on"], len(got["generic"])))
    assert sorted(got) == sorted(gold)
    for key in sorted(gold):
        assert got[key] == gold[key], (key, got[key], gold[key])
    # flags were compared: tiers do overflow in these inputs, with the over(32) of the moved checks among the reasons (no window of w24_k14 leaves its first tier)
    assert name == "w24_k14" or (got["over_events"] > 100 and any("0x20" in b for b in got["over_bits"].values()))

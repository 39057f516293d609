"""One context, many batches of different shapes: what a device worker of daccord_hip does for a whole run, and what bench.py's resident re-runs
do, through the C ABI.  Every other device test builds a fresh Engine for one batch; the state that outlives a batch -- the stages' run flags and
input lists, buffers that grow and move, the hand-over buffer that appears at the second use, the shared slab of the gw tiers, slabs of the trailing
stages allocated by whichever batch needs them first, per-batch launch settings, a second dacc_set_error_profile / dacc_load_db -- is only seen by
running a context through changes of shape.  Steps and sequences: tests/lifecycle_cases.py.

After EVERY step of a sequence:
  parity    window records, fragments and FASTA equal the live oracle's, every pile's status is 0 and there is no message
  rerun     dacc_rerun_resident gives the same fragments and the same integer counters as the pass before it
  counters  every integer field of dacc_timing equals that field of a FRESH context that ran only this step, taken from the fresh context's rerun
            (so that both contexts have the hand-over buffer); a stage or tier time is zero in one exactly if it is zero in the other.  No field
            is exempt: none of the counters depends on the capacity of the hand-over buffer (a window that finds no free slot restarts from its
            strings in the next tier and is counted on the same lists)
  nothing   a step that launches no window kernel (Z, N0, WZ) returns no fragment, zero in every counter and 0.0 in every stage and tier time,
            whatever ran before it
  again     a shape that comes back later in the same context gives bit-identical fragments and identical integer counters
and the premises of the steps, taken from the fresh contexts, so that a changed generator fails loudly instead of testing nothing.

first_tier is not a counter but the name of the first slot's kernel (include/daccord_hip.h: 1 or 4, never 0): it is compared with the fresh
context's in every step, the steps that launch nothing included, where it is 1.
The phase times between the events of a pass (h2d, trace, window, vote, emit, d2h, total) are no stage's or tier's: they are not compared.
No assertion is on an absolute time.  The checks of a sequence are collected and asserted together, so that one run shows every step's findings.
Run with -m gpu."""
import time
import numpy as np
import pytest
import pyoracle
import lifecycle_cases as LF
import longstr_cases
from daccord_amd import engine
from common import windows_equal, frags_equal

pytestmark = pytest.mark.gpu

COUNTERS = ["nwindows", "nblocks", "tier0_in", "tier0_out", "tier7_in", "tier7_out", "tier10_ran", "tier10_out", "long_windows", "long_first_tier",
            "deep_windows", "deep_out", "last_windows", "last_out", "vdeep_windows", "vdeep_out", "xdeep_windows", "xdeep_out", "longstr_windows", "longstr_out"]
STAGE_MS = ["tier0_ms", "tier7_ms", "tier10_ms", "deep_ms", "last_ms", "vdeep_ms", "xdeep_ms", "longstr_ms"]
ENV = ("DACC_TIERS", "DACC_NOFAST", "DACC_HAND", "DACC_SCHED", "DACC_LAST_TIER", "DACC_VDEEP_TIER", "DACC_XDEEP_TIER", "DACC_DEEP_TIER", "DACC_DENSE_TIER",
       "DACC_LAST_AS_SLOT2", "DACC_VDEEP_AS_SLOT2", "DACC_XDEEP_AS_SLOT2", "DACC_WIDE_TIER", "DACC_LONGSTR_TIER", "DACC_LONG128", "DACC_T0INST", "DACC_T7INST",
       "DACC_T7_ADAPT", "DACC_DEBUG_RETRY", "DACC_FEAS_NEED", "DACC_TRACE_DYN")


def _ints(t):
    """every integer field of the record that says what ran: {name: value}, tier_out[i] as tier_out0 ... 2, and first_tier"""
    r = {f: int(getattr(t, f)) for f in COUNTERS}
    r.update({"tier_out%d" % i: int(t.tier_out[i]) for i in range(3)})
    r["first_tier"] = int(t.first_tier)
    return r


def _ms(t):
    r = {f: float(getattr(t, f)) for f in STAGE_MS}
    r.update({"tier_ms%d" % i: float(t.tier_ms[i]) for i in range(3)})
    return r


def _diff(a, b):
    return {k: (a[k], b[k]) for k in a if a[k] != b[k]}


def _prepare(E, s, loaded):
    """the setup calls a step needs on a context in state `loaded` = [data key, profile]: a changed profile before a changed read database"""
    if loaded[1] != s.profile:
        E.set_error_profile(*s.profile); loaded[1] = s.profile
    if loaded[0] != s.data:
        E.load_db(s.d.bps, s.d.boff, s.d.rlen); loaded[0] = s.data


def _submit(E, s):
    return E(s.piles, s.ovl, s.trace, trace_bytes=s.trace_bytes)


_fresh = {}


def fresh(name, switch):
    """(integer counters, stage and tier times) of the rerun pass of a fresh context that ran only this step: the reference of the counter checks,
    once per process and switch setting"""
    if (name, switch) not in _fresh:
        s = LF.step(name)
        E = engine.Engine(LF.params(name))
        _prepare(E, s, [None, None])
        _submit(E, s)
        E.rerun(); E.collect()
        t = E.timing_long()
        _fresh[(name, switch)] = (_ints(t), _ms(t))
        E.close()
    return _fresh[(name, switch)]


def _premises(seq, switch):
    """without these a sequence tests nothing"""
    F = {n: fresh(n, switch)[0] for n in set(seq)}
    if "D50" in F: assert F["D50"]["first_tier"] == 4
    if "S1" in F: assert F["S1"]["first_tier"] == 1
    if "M" in F: assert F["M"]["vdeep_windows"] == 131
    if "P" in F: assert F["P"]["xdeep_windows"] > 0
    if "W100" in F: assert F["W100"]["longstr_windows"] == longstr_cases.FINISHED["W100"]
    if "S2" in F and "S1" in F: assert F["S2"]["nwindows"] > F["S1"]["nwindows"]
    for n in LF.LAUNCH_NOTHING:
        if n in F: assert F[n]["nwindows"] == 0


def run_sequence(seqname, monkeypatch, switch=None):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if switch:
        monkeypatch.setenv(*switch)      # (dacc_create reads the switches: set before any Engine is built)
    seq = LF.SEQUENCES[seqname]
    _premises(seq, switch)
    bad = []      # every finding of the sequence: (position, step, what)
    E = engine.Engine(LF.params(seq[0]))
    loaded = [None, None]; seen = {}
    t0 = time.perf_counter()
    for pos, name in enumerate(seq):
        s = LF.step(name)
        wo, fo, bo = LF.oracle(name)
        fint, fms = fresh(name, switch)
        say = lambda what, pos=pos, name=name: bad.append("step %d (%s): %s" % (pos, name, what))
        tstep = time.perf_counter()
        _prepare(E, s, loaded)
        fx, bx = _submit(E, s)
        # parity
        wx = E.debug_windows(); t = E.timing_long(); ints = _ints(t); ms = _ms(t)
        if windows_equal(wo, wx) != []: say("window records differ from the oracle's: %s" % windows_equal(wo, wx)[:8])
        if not frags_equal(fo, bo, fx, bx): say("fragments differ from the oracle's (%d / %d)" % (len(fx), len(fo)))
        if engine.fasta(fx, bx) != pyoracle.fasta(fo, bo): say("FASTA differs from the oracle's")
        status, msgs = E.pile_status()
        if len(status) != len(s.piles) or status.any() or msgs: say("pile status %s, messages %s" % (list(status), msgs))
        # rerun
        E.rerun(); f2, b2 = E.collect(); t2 = E.timing_long(); ints2 = _ints(t2); ms2 = _ms(t2)
        if not (f2.tobytes() == fx.tobytes() and b2 == bx): say("the rerun's fragments differ from the first pass's")
        if ints2 != ints: say("the rerun's counters differ from the first pass's (first, rerun): %s" % _diff(ints, ints2))
        # counters against the fresh context's: both passes of the aged context
        for what, got, gotms in (("first pass", ints, ms), ("rerun", ints2, ms2)):
            if got != fint: say("%s: counters differ from the fresh context's (aged, fresh): %s" % (what, _diff(got, fint)))
            z = {k: (gotms[k], fms[k]) for k in fms if (gotms[k] == 0.0) != (fms[k] == 0.0)}
            if z: say("%s: times that are zero in one context only (aged, fresh): %s" % (what, z))
            if name in LF.LAUNCH_NOTHING:
                nz = {k: v for k, v in got.items() if v and k != "first_tier"}
                nz.update({k: v for k, v in gotms.items() if v != 0.0})
                if nz: say("%s: launches nothing, but reports %s" % (what, nz))
        if name in LF.LAUNCH_NOTHING and (len(fx) or len(bx)): say("launches nothing, but returns %d fragments" % len(fx))
        # a shape that comes back
        if name in seen:
            f1, b1, i1 = seen[name]
            if not (f1.tobytes() == fx.tobytes() and b1 == bx): say("fragments differ from the first time the context ran this step")
            if i1 != ints: say("counters differ from the first time the context ran this step (then, now): %s" % _diff(i1, ints))
        else:
            seen[name] = (fx, bx, ints)
        print("lifecycle %s%s step %d %-4s %.2f s: %s" % (seqname, " %s=%s" % switch if switch else "", pos, name, time.perf_counter() - tstep,
                                                          {k: v for k, v in ints.items() if v}))
    E.close()
    print("lifecycle %s%s: steps %s, %.2f s with the oracle's and the fresh contexts' share" % (seqname, " %s=%s" % switch if switch else "", seq, time.perf_counter() - t0))
    assert bad == [], "\n".join(bad)


def test_sequence_a_shallow_first(monkeypatch):
    """S1, S2, D50, M, Z, P, N0, S1', S1: buffers grow step by step, the hand-over buffer appears at S2, the chain switches at D50, the trailing stages'
    slabs are allocated at M and P, two steps launch nothing right behind the deepest ones, the profile changes and comes back"""
    run_sequence("A", monkeypatch)


def test_sequence_b_deepest_first(monkeypatch):
    """P, Z, M, D50, S1, S2, Z, P: slabs and the largest buffers first, so later batches never reallocate; the deepest stage runs twice with other work between"""
    run_sequence("B", monkeypatch)


def test_sequence_c_wide(monkeypatch):
    """W0, W100, WZ, W0, W100 at w = 100: the long string stage's slab and hand-on lists are allocated at the second step; the stage reports zeros in W0 behind W100"""
    run_sequence("C", monkeypatch)


@pytest.mark.parametrize("switch", LF.SWITCHES_D, ids=lambda s: "%s=%s" % s)
def test_sequence_d_switches(switch, monkeypatch):
    """sequence A's first six steps without the hand-over buffer, and with the generic engine's work counter"""
    run_sequence("D", monkeypatch, switch)

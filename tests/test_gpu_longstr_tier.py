"""The long string stage on the device, through the C ABI: k_window_fast<17> (four words per pattern mask, strings of up to 255 bases, layout and
slab in one buffer of device memory per workgroup) runs on the second stream of a wide batch over the windows with a B string of more than 128 bases
and hands on to the generic engine of that stream.  Per-window records, fragments and FASTA equal the live oracle with the stage and without it
(DACC_LONGSTR_TIER=0), and longstr_ms / longstr_windows / longstr_out, the 16 bytes appended to dacc_timing, say where the windows finished.
Shapes: tests/longstr_cases.py; the emulation's counts for them: tests/test_longstr_tier.py.  Run with -m gpu."""
import ctypes as C
import pytest
import pyoracle
import longstr_cases as LC
from daccord_amd import engine
from daccord_amd._structs import DaccTiming, DaccTimingLong, default_params
from common import windows_equal, frags_equal

pytestmark = pytest.mark.gpu


def _engine(name, monkeypatch, **env):
    for k in ("DACC_TIERS", "DACC_LAST_TIER", "DACC_LAST_AS_SLOT2", "DACC_WIDE_TIER", "DACC_LONGSTR_TIER"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = LC.shape(name)[0]
    E = engine.Engine(LC.params(name)); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    return E


def _run_and_check(name, E):
    d, ovl, sel, tr, tb = LC.shape(name)
    fx, bx = E(sel, ovl, tr, trace_bytes=tb)
    wo, fo, bo = LC.oracle(name)
    LC.check(name, wo)
    t = E.timing_long()
    print("long string stage %s: windows %d, long_windows %d, longstr_windows %d, longstr_out %d, longstr_ms %.3f, last_windows %d, last_out %d, window_ms %.2f" %
          (name, len(wo), t.long_windows, t.longstr_windows, t.longstr_out, t.longstr_ms, t.last_windows, t.last_out, t.window_ms))
    assert windows_equal(wo, E.debug_windows()) == [] and frags_equal(fo, bo, fx, bx)
    assert engine.fasta(fx, bx) == pyoracle.fasta(fo, bo)
    return t


@pytest.mark.parametrize("name", ["N120", "W64", "S", "S2"])
def test_stage_equals_the_oracle_and_counts_what_the_emulation_counts(name, monkeypatch):
    E = _engine(name, monkeypatch)
    t = _run_and_check(name, E)
    assert t.long_windows > 0 and t.longstr_windows + t.longstr_out == t.long_windows
    assert t.longstr_windows == LC.FINISHED[name]
    assert t.longstr_ms > 0
    # the same batch again: same fragments, same counters
    fo, bo = LC.oracle(name)[1:]
    E.rerun(); f2, b2 = E.collect(); t2 = E.timing_long()
    assert frags_equal(fo, bo, f2, b2)
    assert (t2.long_windows, t2.longstr_windows, t2.longstr_out) == (t.long_windows, t.longstr_windows, t.longstr_out) and t2.longstr_ms > 0
    E.close()


def test_second_batch_on_the_same_context(monkeypatch):
    """other piles on the context that has run the stage (its slab and hand-on lists are the context's)"""
    E = _engine("N120", monkeypatch)
    t = _run_and_check("N120", E)
    d, ovl, sel, tr, tb = LC.shape("N120")
    more = LC.other_piles("N120", 1)
    assert len(more) == 1
    fx, bx = E(more, ovl, tr, trace_bytes=tb)
    O = pyoracle.Oracle(LC.params("N120")); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
    fo, bo = O.run(more, ovl, tr, trace_bytes=tb, nthreads=8, want_windows=True)
    t2 = E.timing_long()
    assert windows_equal(O.windows(), E.debug_windows()) == [] and frags_equal(fo, bo, fx, bx)
    assert t2.long_windows > 0 and t2.longstr_windows + t2.longstr_out == t2.long_windows and t2.longstr_ms > 0
    assert t2.nwindows != t.nwindows      # the record is the second batch's
    E.close()


@pytest.mark.parametrize("name", ["N120", "S2"])
def test_switch_off_restores_the_generic_engine_alone(name, monkeypatch):
    E = _engine(name, monkeypatch, DACC_LONGSTR_TIER="0")
    t = _run_and_check(name, E)
    assert (t.longstr_ms, t.longstr_windows, t.longstr_out) == (0.0, 0, 0)
    assert t.long_windows == {"N120": 73, "S2": 37}[name]      # the second stream read what it reads with the stage (S2: 36 finish there, one is handed on)
    E.close()


def test_wide_batch_without_a_long_string_does_not_run_the_stage(monkeypatch):
    E = _engine("W96", monkeypatch)
    t = _run_and_check("W96", E)
    assert LC.LISTLEN["W96"] == 0 and t.long_windows == 0
    assert (t.longstr_ms, t.longstr_windows, t.longstr_out) == (0.0, 0, 0)
    E.close()


def test_narrow_batch_does_not_run_the_stage(monkeypatch):
    """the smoke shape (w = 40): the second stream's tier is tier 5 inside k_window_long, as before"""
    from daccord_amd.synth import SynthData
    for k in ("DACC_TIERS", "DACC_LONGSTR_TIER"):
        monkeypatch.delenv(k, raising=False)
    d = SynthData(60000, 150, 3000, seed=2)
    ovl, piles = engine.pile_select(d.ovl, d.piles)
    p = default_params(k=8)
    E = engine.Engine(p); E.set_error_profile(*d.error_profile()); E.load_db(d.bps, d.boff, d.rlen)
    fx, bx = E(piles[:6], ovl, d.trace)
    O = pyoracle.Oracle(p); O.set_error_profile(*d.error_profile()); O.load_db(d.bps, d.boff, d.rlen)
    fo, bo = O.run(piles[:6], ovl, d.trace, nthreads=8)
    assert engine.fasta(fx, bx) == pyoracle.fasta(fo, bo)
    t = E.timing_long()
    assert (t.longstr_ms, t.longstr_windows, t.longstr_out) == (0.0, 0, 0)
    E.close()


def test_timing_record_sizes(monkeypatch):
    """dacc_last_timing2 copies what the caller has room for: with the 176 bytes of the record before the stage, bytes 176 ... 191 of the caller's
    buffer stay as they were; with 192 they are the stage's fields"""
    assert C.sizeof(DaccTiming) == 176 and C.sizeof(DaccTimingLong) == 192
    E = _engine("W64", monkeypatch)
    _run_and_check("W64", E)
    buf = (C.c_uint8 * 192)(*([0xA5] * 192))
    E._chk(E.L.dacc_last_timing2(E.h, C.byref(buf), 176))
    assert bytes(buf[176:192]) == b"\xa5" * 16 and bytes(buf[:176]) != b"\xa5" * 176
    E._chk(E.L.dacc_last_timing2(E.h, C.byref(buf), 192))
    t = DaccTimingLong.from_buffer_copy(bytes(buf))
    assert t.longstr_windows == LC.FINISHED["W64"] and t.pad2_ == 0 and t.longstr_ms > 0
    assert bytes(buf[:176]) == bytes(E.timing())
    E.close()

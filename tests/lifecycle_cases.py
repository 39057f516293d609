"""Steps and sequences of the context-lifecycle tests (tests/test_gpu_context_lifecycle.py on the device, the planner's share of them in
tests/test_plan.py): ONE context is fed batches of different shapes one after the other, the way a device worker of daccord_hip feeds its
context whatever the read range holds.  A step is (data set, piles, overlaps, trace, bytes per trace value, error profile); its oracle result
-- (windows, fragments, bases) -- is computed once per process, shared and never modified.  The large shapes and their oracles are those of
tests/vdeep_cases.py, tests/xdeep_cases.py and tests/longstr_cases.py: nothing new and large is generated here.

narrow context, k = 14, every other parameter at its default:
  S1    SynthData(100000, 200, 5000, seed=1) (conftest.small_data's set), piles[:4]: the shallow chain
  S2    the same set, piles[4:10]: more windows than S1, so the buffers grow; the second use of a context, so the hand-over buffer appears
  D50   SynthData(30000, 300, 5000, seed=7), piles[10:12]: the deep chain (first_tier == 4)
  M     vdeep_cases.shape("M"): 247 windows of 23 ... 291 strings; tier 12, the last stage and the very deep stage run
  P     xdeep_cases.shape("P"): 37 windows of 447 ... 1932 strings; the deepest stage runs
  Z     S1's piles with every novl set to 0: no window, no fragment
  N0    no pile at all
  S1p   S1 under the error profile (0.05, 0.05, 0.85) instead of the data's: another table support, so other LDS sizes and slab strides
wide context, k = 8, w = 100, a = 25 (longstr_cases.params("W100")), on S1's data set:
  W0    piles[2:4] with the plain trace
  W100  longstr_cases.shape("W100"): the long string stage runs
  WZ    W0's piles with every novl set to 0

A sequence is a list of steps for one context.  Between two steps the caller loads the read database again when `data` changes and sets the
error profile again when `profile` changes."""
import collections
import pyoracle
import vdeep_cases
import xdeep_cases
import longstr_cases
from daccord_amd._structs import default_params
from daccord_amd.synth import SynthData

PROFILE_OTHER = (0.05, 0.05, 0.85)

SEQUENCES = {
    "A": ["S1", "S2", "D50", "M", "Z", "P", "N0", "S1p", "S1"],      # shallow first
    "B": ["P", "Z", "M", "D50", "S1", "S2", "Z", "P"],               # deepest first: slabs and the largest buffers before anything else
    "C": ["W0", "W100", "WZ", "W0", "W100"],                         # wide
}
SEQUENCES["D"] = SEQUENCES["A"][:6]                                   # A's first six steps, under a switch read by dacc_create
SWITCHES_D = [("DACC_HAND", "0"), ("DACC_SCHED", "3")]                # no hand-over buffer; the generic engine draws its windows from a counter too (default 1)
WIDE = ("W0", "W100", "WZ")
LAUNCH_NOTHING = ("Z", "N0", "WZ")

# data: a key that says which read database the step needs (equal keys: the same reads)
Step = collections.namedtuple("Step", "name data d ovl piles trace trace_bytes profile")

_sets = {}
_steps = {}
_oracle = {}


def params(name):
    """the parameters of the context a step belongs to"""
    return longstr_cases.params("W100") if name in WIDE else default_params(k=14)


def _set(key):
    if key not in _sets:
        d = SynthData(100000, 200, 5000, seed=1) if key == "small" else SynthData(30000, 300, 5000, seed=7)
        ovl, piles = pyoracle.pile_select(d.ovl, d.piles)
        _sets[key] = (d, ovl, piles)
    return _sets[key]


def _zero(piles):
    p = piles.copy()
    p["novl"] = 0
    return p


def step(name):
    if name in _steps:
        return _steps[name]
    if name in ("S1", "S2", "Z", "N0", "S1p", "W0", "WZ"):
        d, ovl, piles = _set("small")
        sel = {"S1": piles[:4], "S2": piles[4:10], "Z": _zero(piles[:4]), "N0": piles[:0], "S1p": piles[:4], "W0": piles[2:4], "WZ": _zero(piles[2:4])}[name]
        s = Step(name, "small", d, ovl, sel, d.trace, d.trace_bytes, PROFILE_OTHER if name == "S1p" else tuple(d.error_profile()))
    elif name == "D50":
        d, ovl, piles = _set("d50")
        s = Step(name, "d50", d, ovl, piles[10:12], d.trace, d.trace_bytes, tuple(d.error_profile()))
    elif name == "M":
        d, ovl, sel = vdeep_cases.shape("M")
        s = Step(name, "M", d, ovl, sel, d.trace, d.trace_bytes, tuple(d.error_profile()))
    elif name == "P":
        d, ovl, sel = xdeep_cases.shape("P")
        s = Step(name, "P", d, ovl, sel, d.trace, d.trace_bytes, tuple(d.error_profile()))
    elif name == "W100":
        # (its data set is S1's: SHAPES["W100"]["synth"]; the overlaps are the same selection, the trace is warped)
        d, ovl, sel, tr, tb = longstr_cases.shape("W100")
        assert longstr_cases.SHAPES["W100"]["synth"] == dict(genome_len=100000, nreads=200, read_len=5000, seed=1)
        s = Step(name, "small", d, ovl, sel, tr, tb, tuple(d.error_profile()))
    else:
        raise KeyError(name)
    _steps[name] = s
    return s


def oracle(name, nthreads=8):
    """(windows, fragments, bases) of the oracle for a step, and the shape module's premises where it has them"""
    if name not in _oracle:
        if name == "M":
            r = vdeep_cases.oracle("M", k=14, nthreads=nthreads); vdeep_cases.check("M", r[0])
        elif name == "P":
            r = xdeep_cases.oracle("P", k=14, nthreads=nthreads); xdeep_cases.check("P", r[0])
        elif name == "W100":
            r = longstr_cases.oracle("W100", nthreads=nthreads); longstr_cases.check("W100", r[0])
        else:
            s = step(name)
            O = pyoracle.Oracle(params(name)); O.set_error_profile(*s.profile); O.load_db(s.d.bps, s.d.boff, s.d.rlen)
            fo, bo = O.run(s.piles, s.ovl, s.trace, trace_bytes=s.trace_bytes, nthreads=nthreads, want_windows=True)
            r = (O.windows(), fo, bo)
        if name in LAUNCH_NOTHING:
            assert len(r[0]) == 0 and len(r[1]) == 0 and len(r[2]) == 0, name
        _oracle[name] = r
    return _oracle[name]

"""bench.py --dump-outputs on the host: what the last timed step returned, written as float arrays that two builds can compare
output for output -- every fragment field, an exact per-fragment checksum of the bases, a seeded sample of the base buffer -- and
never more than the budget (64 MB by default)."""
import os

import numpy as np

import bench
from daccord_amd._structs import DaccFragment


def _result(nf, seed=1):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 3000, nf)
    fr = np.zeros(nf, dtype=np.dtype(DaccFragment))
    fr["aread"] = np.arange(nf) // 3; fr["first"] = rng.integers(0, 9000, nf); fr["len"] = lens; fr["last"] = fr["first"] + lens
    fr["seq_off"] = np.concatenate([[0], np.cumsum(lens)[:-1]])
    ba = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(lens.sum())).tobytes()
    return fr, ba


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_complete_exact_and_repeatable(tmp_path):
    fr, ba = _result(500)
    bench.dump_outputs(str(tmp_path / "a"), fr, ba)
    bench.dump_outputs(str(tmp_path / "b"), fr, ba)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    for f in ("aread", "first", "last", "len", "seq_off"):
        assert np.array_equal(a["fragment_" + f], fr[f].astype(np.float64))
    # small enough: the sample is the whole base buffer, in order
    assert np.array_equal(a["bases_sample"], np.frombuffer(ba, np.uint8).astype(np.float32))
    j = 7; o, n = int(fr["seq_off"][j]), int(fr["len"][j])
    assert a["fragment_base_checksum"][j] == sum((i + 1) * c for i, c in enumerate(ba[o:o + n]))
    # one changed base changes its fragment's checksum and nothing else
    k = int(fr["seq_off"][3]) + 1
    bb = bytearray(ba); bb[k] = ord("A") if bb[k] != ord("A") else ord("C")
    bench.dump_outputs(str(tmp_path / "c"), fr, bytes(bb))
    c = _load(tmp_path / "c")
    diff = np.nonzero(c["fragment_base_checksum"] != a["fragment_base_checksum"])[0]
    assert list(diff) == [3]


def test_dump_stays_within_its_budget(tmp_path):
    fr, ba = _result(4000)
    budget = 1 << 18
    sizes = bench.dump_outputs(str(tmp_path / "a"), fr, ba, budget=budget)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= budget + 128 * len(sizes)             # + the .npy headers
    a = _load(tmp_path / "a")
    assert 0 < len(a["fragment_index"]) < len(fr) and 0 < len(a["bases_sample"]) < len(ba)
    idx = a["fragment_index"].astype(np.int64)
    assert np.array_equal(a["fragment_len"], fr["len"][idx].astype(np.float64))
    bench.dump_outputs(str(tmp_path / "b"), fr, ba, budget=budget)
    b = _load(tmp_path / "b")
    assert all(np.array_equal(a[k], b[k]) for k in a)

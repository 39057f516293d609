"""Case table and numpy references of the wavefront primitive probe (tests/test_waveprobe.py: 64-lane host wavefront,
tests/test_gpu_waveprobe.py: gfx950).  Both files run the same checks on a waveprobe_lib.Probe; the expected values are computed here
with plain numpy / Python integers, never with the host emulation.  Everything is integer: every comparison is exact equality.

The inputs are seeded and built once per process; nothing modifies them."""
import functools
import numpy as np
import waveprobe_lib as WL

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
# the row (16 lanes) and bank (32 lanes) seams of the DPP scan sequence: row_shr stays inside a row, row_bcast15 / row_bcast31 cross them
SEAMS = (0, 15, 16, 31, 32, 47, 48, 63)
LANES = np.arange(64)

# (CAP, R32) of wv_sort_keys<CAP,R32> in the product, in the order of the probe's sort modes (probe_body.hpp: WP_SORT_PAIRS):
# FastLds<CT>::keycap = pow2(maxs), CT::precap, pow2(CT::scap) over the FastTier table of fast_window.hpp, and tier 4's R32
SORT_PAIRS = [(32, False), (64, False), (128, False), (256, False), (512, False), (576, False), (704, False), (1024, False), (2048, False),
              (2560, False), (3072, False), (4096, False), (8192, False), (16384, False), (2048, True)]
MODE_BITONIC, MODE_BITONIC_N, NMODES = 15, 16, 17
MAXN = 16384
# every size at which wv_sort_keys changes its network (128 / 256 / 512 / 1024 / 2048), one below and one above, and the wavefront's own seams
SORT_SIZES = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)


def mode_name(m):
    return "bitonic" if m == MODE_BITONIC else ("bitonic_n" if m == MODE_BITONIC_N else "keys<%d%s>" % (SORT_PAIRS[m][0], ",R32" if SORT_PAIRS[m][1] else ""))


def _same(got, want, what):
    got = np.asarray(got, np.uint64); want = np.asarray(want, np.uint64)
    if got.shape != want.shape or not (got == want).all():
        bad = np.argwhere(got != want)[:6].tolist() if got.shape == want.shape else "shape"
        raise AssertionError("%s: %s\n got  %s\n want %s" % (what, bad, [hex(int(x)) for x in got.ravel()[:64]], [hex(int(x)) for x in want.ravel()[:64]]))


# ---- 32 bit scans, reductions, votes ----
@functools.lru_cache(None)
def u32_cases():
    rng = np.random.default_rng(11)
    vals = [("zero", np.zeros(64, np.uint32)), ("all_ones", np.full(64, M32, np.uint32))]
    for s in SEAMS:
        v = np.zeros(64, np.uint32); v[s] = 0xDEADBEEF; vals.append(("single@%d" % s, v))
        v = np.zeros(64, np.uint32); v[s] = 1; vals.append(("one@%d" % s, v))
    vals.append(("bit31", (rng.integers(0, 1 << 31, 64, dtype=np.uint64) | (1 << 31)).astype(np.uint32)))
    vals.append(("bit31_only", np.full(64, 1 << 31, np.uint32)))
    vals.append(("lane_plus_1", (LANES + 1).astype(np.uint32)))
    vals.append(("small", rng.integers(0, 1000, 64, dtype=np.uint64).astype(np.uint32)))
    for i in range(3):
        vals.append(("random%d" % i, rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)))
    flags = [("all", np.ones(64, np.uint32)), ("none", np.zeros(64, np.uint32)), ("even", (LANES % 2 == 0).astype(np.uint32)),
             ("odd", (LANES % 2 == 1).astype(np.uint32)), ("low32", (LANES < 32).astype(np.uint32)), ("high32", (LANES >= 32).astype(np.uint32))]
    for s in SEAMS:
        f = np.zeros(64, np.uint32); f[s] = 1; flags.append(("flag@%d" % s, f))
        f = np.ones(64, np.uint32); f[s] = 0; flags.append(("hole@%d" % s, f))
    for i in range(2):
        flags.append(("randomflags%d" % i, rng.integers(0, 2, 64, dtype=np.uint64).astype(np.uint32)))
    flags[0] = ("all_nonzero_values", np.full(64, 0x80, np.uint32))      # a predicate is any non-zero value
    n = max(len(vals), len(flags))
    names = ["%s/%s" % (vals[i % len(vals)][0], flags[i % len(flags)][0]) for i in range(n)]
    V = np.stack([vals[i % len(vals)][1] for i in range(n)]); F = np.stack([flags[i % len(flags)][1] for i in range(n)])
    V.setflags(write=False); F.setflags(write=False)
    return names, V, F


def expected_u32(v, f):
    """{field: 64 values} for one wavefront of values v and predicates f"""
    v = v.astype(np.uint64); p = (f != 0).astype(np.uint64)
    inc = np.cumsum(v, dtype=np.uint64)                       # < 2^38: exact in uint64
    pinc = np.cumsum(p, dtype=np.uint64)
    ballot = sum(1 << int(l) for l in LANES if p[l])
    one = np.ones(64, np.uint64)
    return {"scan_pre": (inc - v) & np.uint64(M32), "scan_tot": one * (inc[-1] & np.uint64(M32)), "sum": one * (inc[-1] & np.uint64(M32)),
            "max": one * v.max(), "or": one * np.bitwise_or.reduce(v), "flag_pre": pinc - p, "flag_tot": one * pinc[-1],
            "ballot": one * np.uint64(ballot), "any": one * np.uint64(1 if p.any() else 0),
            "lanemask_lt": np.array([(1 << int(l)) - 1 for l in LANES], np.uint64)}


def check_u32(P):
    names, V, F = u32_cases()
    out = P.u32(V, F)
    for c, name in enumerate(names):
        E = expected_u32(V[c], F[c])
        for fi, field in enumerate(WL.F32):
            _same(out[c, fi], E[field], "%s of case %s" % (field, name))


# ---- 64 bit reductions ----
@functools.lru_cache(None)
def u64_cases():
    rng = np.random.default_rng(12)
    r32 = lambda: rng.integers(0, 1 << 32, 64, dtype=np.uint64)
    cases = [("zero", np.zeros(64, np.uint64)), ("all_ones", np.full(64, M64, np.uint64)),
             ("high_word_only", (r32() << np.uint64(32)) | np.uint64(0x12345678)), ("low_word_only", (np.uint64(0x9ABCDEF0) << np.uint64(32)) | r32()),
             ("high_word_only_low_ones", (r32() << np.uint64(32)) | np.uint64(M32)), ("low_word_only_high_ones", (np.uint64(M32) << np.uint64(32)) | r32())]
    for s in (0, 31, 32, 63):
        v = np.zeros(64, np.uint64); v[s] = M64; cases.append(("max@%d" % s, v))
        v = np.full(64, M64, np.uint64); v[s] = 0; cases.append(("zero@%d" % s, v))
        v = np.full(64, 1 << 32, np.uint64); v[s] = (1 << 32) - 1; cases.append(("below_word_seam@%d" % s, v))
    for i in range(3):
        cases.append(("random%d" % i, rng.integers(0, 1 << 64, 64, dtype=np.uint64)))
    V = np.stack([c[1] for c in cases]); V.setflags(write=False)
    return [c[0] for c in cases], V


def check_u64(P):
    names, V = u64_cases()
    out = P.u64(V)
    for c, name in enumerate(names):
        v = [int(x) for x in V[c]]
        E = {"sum64": sum(v) & M64, "max64": max(v), "min64": min(v), "or64": int(np.bitwise_or.reduce(V[c])), "uni64": v[0]}
        for fi, field in enumerate(WL.F64):
            _same(out[c, fi], np.full(64, E[field], np.uint64), "%s of case %s" % (field, name))


# ---- broadcasts and shuffles ----
@functools.lru_cache(None)
def xlane_cases():
    rng = np.random.default_rng(13)
    perms = [("identity", LANES.copy()), ("reverse", 63 - LANES)] + [("xor%d" % m, LANES ^ m) for m in (1, 2, 4, 8, 16, 32)]
    perms += [("xor63", LANES ^ 63), ("rotate1", (LANES + 1) % 64), ("rotate17", (LANES + 17) % 64)]
    perms += [("random_perm%d" % i, rng.permutation(64)) for i in range(2)]
    perms += [("all_from_%d" % s, np.full(64, s)) for s in SEAMS]
    perms += [("random_sources", rng.integers(0, 64, 64))]
    n = len(perms)
    bsrc = np.array([SEAMS[i % len(SEAMS)] for i in range(n)], np.int32)
    names = ["%s/bcast_from_%d" % (perms[i][0], bsrc[i]) for i in range(n)]
    src = np.stack([p[1] for p in perms]).astype(np.int32)
    v32 = rng.integers(0, 1 << 32, (n, 64), dtype=np.uint64).astype(np.uint32); v64 = rng.integers(0, 1 << 64, (n, 64), dtype=np.uint64)
    v32[0, :] |= 1 << 31; v64[1, :] |= np.uint64(1 << 63)
    for a in (src, bsrc, v32, v64):
        a.setflags(write=False)
    return names, v32, v64, src, bsrc


def check_xlane(P):
    names, v32, v64, src, bsrc = xlane_cases()
    out = P.xlane(v32, v64, src, bsrc)
    for c, name in enumerate(names):
        E = {"bcast": np.full(64, v32[c, bsrc[c]]), "bcast64": np.full(64, v64[c, bsrc[c]]), "uni": np.full(64, v32[c, 0]),
             "shfl": v32[c][src[c]], "shfl64": v64[c][src[c]]}
        for fi, field in enumerate(WL.FX):
            _same(out[c, fi], E[field], "%s of case %s" % (field, name))


# ---- sorts ----
def sort_sizes(mode):
    if mode == MODE_BITONIC:
        return [0, 1] + [1 << i for i in range(1, 15)]            # powers of two up to 16384
    cap = MAXN if mode == MODE_BITONIC_N else SORT_PAIRS[mode][0]
    return sorted(set(min(n, cap) for n in SORT_SIZES + (cap - 1, cap)))


KEYSETS = ("distinct_both_words", "random64", "descending", "one_key_all_ones")


def _keys(rng, kind, n):
    if kind == "distinct_both_words":
        return rng.permutation(n).astype(np.uint64) * np.uint64(0x100000001)
    if kind == "random64":
        return rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if kind == "descending":
        return np.sort(rng.integers(0, 1 << 64, n, dtype=np.uint64))[::-1].copy()
    k = rng.integers(0, 1 << 63, n, dtype=np.uint64)               # the value the register sorts pad with, once, among smaller keys
    if n:
        k[rng.integers(0, n)] = M64
    return k


@functools.lru_cache(None)
def sort_cases(mode):
    """(jobs, keys, sorted keys, names) of one sort mode: every size x every key set, each job its own slice of one key buffer"""
    rng = np.random.default_rng(100 + mode)
    jobs, chunks, want, names, off = [], [], [], [], 0
    for n in sort_sizes(mode):
        for kind in KEYSETS:
            k = _keys(rng, kind, n)
            jobs.append((mode, n, off, 0)); chunks.append(k); want.append(np.sort(k)); names.append("%s n=%d %s" % (mode_name(mode), n, kind)); off += n
    keys = np.concatenate(chunks); exp = np.concatenate(want)
    keys.setflags(write=False); exp.setflags(write=False)
    return np.array(jobs, WL.JOB), keys, exp, names


def check_sort(P, mode, space):
    jobs, keys, exp, names = sort_cases(mode)
    got = P.sort(space, jobs, keys)
    if not (got == exp).all():
        for j, name in zip(jobs, names):
            a, b = int(j["off"]), int(j["off"]) + int(j["n"])
            if not (got[a:b] == exp[a:b]).all():
                bad = np.nonzero(got[a:b] != exp[a:b])[0]
                raise AssertionError("%s (%s): %d of %d keys differ from np.sort, first at %d: got %#x want %#x" % (
                    name, "global" if space == WL.SPACE_GLOBAL else "LDS", len(bad), b - a, bad[0], int(got[a + bad[0]]), int(exp[a + bad[0]])))
        raise AssertionError("keys outside every job changed")


@functools.lru_cache(None)
def idx_cases():
    """wv_bitonic_sort_idx: p2 slots (a power of two) holding m indices into nk keys and 0xFFFFFFFF pads, anywhere; keys with many ties"""
    PAD = 0xFFFFFFFF
    rng = np.random.default_rng(14)
    jobs, kch, ich, want, names, koff, ioff = [], [], [], [], [], 0, 0
    for p2 in (1, 2, 4, 64, 128, 256, 1024, 4096):
        for m in sorted(set([0, 1, p2 // 2 + 1, p2 - 1, p2])):
            if m > p2:
                continue
            for kind in ("ties", "all_equal", "distinct"):
                nk = max(m, 1)
                K = (rng.integers(0, 4, nk, dtype=np.uint64) << np.uint64(40)) if kind == "ties" else (
                    np.full(nk, 0x5555555555555555, np.uint64) if kind == "all_equal" else rng.permutation(nk).astype(np.uint64) * np.uint64(0x100000001))
                I = np.full(p2, PAD, np.uint32)
                I[rng.permutation(p2)[:m]] = rng.permutation(m).astype(np.uint32)
                ids = np.arange(m)
                order = ids[np.lexsort((ids, K[:m]))] if m else ids          # by (key, index)
                W = np.full(p2, PAD, np.uint32); W[:m] = order
                jobs.append((p2, nk, koff, ioff)); kch.append(K); ich.append(I); want.append(W); names.append("p2=%d m=%d %s" % (p2, m, kind))
                koff += nk; ioff += p2
    K = np.concatenate(kch); I = np.concatenate(ich); W = np.concatenate(want)
    for a in (K, I, W):
        a.setflags(write=False)
    return np.array(jobs, WL.IDXJOB), K, I, W, names


def check_sort_idx(P, space):
    jobs, K, I, W, names = idx_cases()
    got = P.sort_idx(space, jobs, K, I)
    for j, name in zip(jobs, names):
        a, b = int(j["ioff"]), int(j["ioff"]) + int(j["p2"])
        _same(got[a:b], W[a:b], "wv_bitonic_sort_idx %s" % name)


# ---- atomics ----
def check_atomic(P, init):
    """every lane adds lane+1 and keeps the old value: the old values are the exclusive prefix sums of the additions in SOME order"""
    out = P.atomic(init)
    for r, what in enumerate(("wv_atomic_add on an LDS word", "wv_atomic_add_global", "wv_atomic_add on a global word")):
        old = [(int(x) - init) & M32 for x in out[r, :64]]
        assert int(out[r, 64]) == (init + 2080) & M32, (what, hex(int(out[r, 64])))
        cur = 0
        for lane in sorted(range(64), key=lambda l: old[l]):
            assert old[lane] == cur, (what, "lane %d saw %d, the additions before it sum to %d" % (lane, old[lane], cur))
            cur += lane + 1
        assert cur == 2080

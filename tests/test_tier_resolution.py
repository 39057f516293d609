"""The tier chain as data (daccord_amd/csrc/tier_pipeline.hpp): what readTierSwitches / stageTier / resolveTiers / tierGrid / tierGridGmem make of every
combination of batch shape (shallow, deep, wide), deepest window (0, 250, 251, 1000, 1001, 2001 strings), model table (default profile at w = 40 and
w = 100, one beyond every table capacity) and environment (default; each DACC_*_TIER / DACC_LONG128 /
DACC_HAND switch at 0; every subset of the three DACC_*_AS_SLOT2 switches; DACC_TIERS = 0, 4, 25, 29, 31; equal instance thresholds; DACC_NOFAST=1),
against tests/golden/tier_resolution.txt: 1296 combinations, one line each (switches and flags, then ok, tier and the grid of 37 windows of every stage).  The golden is the output of tests/tiers/tier_resolution.cpp at commit 8be1970 ("Wide batches: strings of
129-255 bases leave the generic engine"), before the trailing stages became rows of TIER_CHAIN; the program uses only names both versions of the header
have, so it compiles unchanged against either.  Host code under AddressSanitizer and UndefinedBehaviorSanitizer, like tests/emit/emit_check.cpp."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "tiers", "tier_resolution.cpp")
_CSRC = os.path.join(os.path.dirname(_HERE), "daccord_amd", "csrc")
_GOLDEN = os.path.join(_HERE, "golden", "tier_resolution.txt")


def test_resolved_chain_equals_the_recorded_one(tmp_path):
    exe = str(tmp_path / "tier_resolution")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-isystem", _CSRC, "-o", exe, _SRC])
    r = subprocess.run([exe], capture_output=True, timeout=300)
    print(r.stderr.decode()[-4000:])
    assert r.returncode == 0 and b"runtime error" not in r.stderr
    want = open(_GOLDEN, "rb").read()
    if r.stdout != want:
        got, exp = r.stdout.split(b"\n"), want.split(b"\n")
        assert len(got) == len(exp), "%d lines, the golden has %d" % (len(got), len(exp))
        for g, e in zip(got, exp):
            assert g == e
    assert r.stdout == want

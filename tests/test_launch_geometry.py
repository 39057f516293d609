"""The launch arithmetic of the batch setup (daccord_amd/csrc/launch_geometry.hpp): the trace kernels' words, lanes, LDS bytes, workgroups per CU and grid, the
generic engine's grids, the hand-over buffer's capacity and the copy size of dacc_last_timing2, against values worked out by hand from the expressions
dacc_submit_piles held inline before the header existed (tests/tiers/launch_geometry.cpp: the arithmetic stands beside each value).  The header alone under
g++ -Wall -Wextra -Werror, host code under AddressSanitizer and UndefinedBehaviorSanitizer, like tests/test_tier_resolution.py."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "tiers", "launch_geometry.cpp")
_CSRC = os.path.join(os.path.dirname(_HERE), "daccord_amd", "csrc")


def test_launch_geometry_equals_the_hand_derived_values(tmp_path):
    alone = str(tmp_path / "alone.cpp")
    open(alone, "w").write('#include "%s"\nint main() { return 0; }\n' % os.path.join(_CSRC, "launch_geometry.hpp"))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", alone])
    src = open(os.path.join(_CSRC, "launch_geometry.hpp")).read()
    assert "hip/" not in src and "getenv" not in src
    exe = str(tmp_path / "launch_geometry")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", _CSRC, "-o", exe, _SRC])
    r = subprocess.run([exe], capture_output=True, timeout=120)
    print(r.stdout.decode()[-8000:]); print(r.stderr.decode()[-4000:])
    assert r.returncode == 0 and b"FAIL" not in r.stdout and b"runtime error" not in r.stderr
    assert b" checks, 0 failed" in r.stdout

"""emitPendingRecord (daccord_amd/csrc/emit_record.hpp): the per-lane routine that turns the pending window record a tier leaves behind into the
final record, as host code under AddressSanitizer and UndefinedBehaviorSanitizer.  tests/emit/emit_check.cpp is a stand-alone program: it runs
the routine on seeded random (A window, consensus) pairs -- m = 1, 2, 24, 40, 63, 64 against n = 0, 1, m-5 .. m+5, 96; unrelated strings, noisy
copies, equal strings, strings over one symbol -- and compares rec[0], the m+2 group offsets and the symbols with a plain O(mn) edit-distance
matrix and the product's traceback priority.  Final and empty records must come back untouched."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emit", "emit_check.cpp")


def test_pending_records_against_the_full_matrix_under_sanitizers(tmp_path):
    exe = str(tmp_path / "emit_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, _SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:]); print(r.stderr[-4000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr

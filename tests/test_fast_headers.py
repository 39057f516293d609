"""The headers the window fast path is cut into (daccord_amd/csrc): fast_tiers.hpp (the rows FastTier<N>, plain C++17), fast_layout.hpp (FastLds<CT>,
fastCapsOf) and fast_window.hpp (the engine).  What the cut is for, as checks: the tier table stands alone, the layout stands on the table and not on
the engine, the planner's translation units do not read the engine, and every layout has the sizes it had before its text moved
(tests/golden/fast_layout_sizes.txt: the output of tests/tiers/fast_layout_sizes.cpp at commit 05b4821, where fast_window.hpp still held all of it).
Host code only; the programs run under AddressSanitizer and UndefinedBehaviorSanitizer like tests/tiers/tier_resolution.cpp."""
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "daccord_amd", "csrc")
_SIZES = os.path.join(_HERE, "tiers", "fast_layout_sizes.cpp")
_RESOLUTION = os.path.join(_HERE, "tiers", "tier_resolution.cpp")
_GOLDEN = os.path.join(_HERE, "golden", "fast_layout_sizes.txt")
_STRICT = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]


def _deps(args):
    """the files a translation unit reads (-M, not -MM: the project's headers are system headers there)"""
    out = subprocess.run(["g++", "-std=c++17", "-M"] + args, check=True, capture_output=True, text=True).stdout
    return {os.path.basename(f) for f in out.replace("\\\n", " ").split(":", 1)[1].split()}


def test_tier_table_compiles_alone():
    """no DACC_EMUL, no device qualifiers, nothing but <cstdint> and tier_pipeline.hpp"""
    hdr = os.path.join(_CSRC, "fast_tiers.hpp")
    subprocess.check_call(["g++"] + _STRICT + ["-fsyntax-only", "-x", "c++", hdr])
    assert re.findall(r'^#include\s+(\S+)', open(hdr).read(), re.M) == ["<cstdint>", '"tier_pipeline.hpp"']
    assert {f for f in _deps(["-x", "c++", hdr]) if f.endswith(".hpp")} == {"fast_tiers.hpp", "tier_pipeline.hpp"}


def test_layout_compiles_alone_without_the_engine():
    """as tests/tiers/tier_resolution.cpp compiles the headers: the 1-lane host build, wave.hpp first, the project's headers as system headers
    (an empty translation unit that includes the two)"""
    args = ["-DDACC_EMUL", "-isystem", _CSRC, "-include", "wave.hpp", "-include", "fast_layout.hpp", "-x", "c++", os.devnull]
    subprocess.check_call(["g++"] + _STRICT + ["-fsyntax-only"] + args)
    assert {f for f in _deps(args) if f.endswith(".hpp")} == {"fast_layout.hpp", "fast_tiers.hpp", "tier_pipeline.hpp", "dev_types.hpp", "wave.hpp"}


def test_planner_units_do_not_read_the_engine():
    deps = _deps(["-isystem", _CSRC, _RESOLUTION])
    assert "fast_layout.hpp" in deps and "fast_tiers.hpp" in deps and "batch_plan.hpp" in deps
    assert "fast_window.hpp" not in deps and "fast_diag.hpp" not in deps and "dbg_window.hpp" not in deps


def test_engine_file_holds_no_table_and_no_layout():
    src = open(os.path.join(_CSRC, "fast_window.hpp")).read()
    assert "struct FastEngine" in src
    assert not re.search(r"struct\s+FastTier<", src) and "FLD(" not in src and not re.search(r"struct\s+Feas", src)


def test_layout_sizes_are_the_recorded_ones(tmp_path):
    exe = str(tmp_path / "fast_layout_sizes")
    subprocess.check_call(["g++", "-O1", "-g"] + _STRICT + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-isystem", _CSRC, "-o", exe, _SIZES])
    r = subprocess.run([exe], capture_output=True, timeout=60)
    print(r.stderr.decode()[-4000:])
    assert r.returncode == 0 and b"runtime error" not in r.stderr
    want = open(_GOLDEN, "rb").read()
    got, exp = r.stdout.split(b"\n"), want.split(b"\n")
    # one line per tier of DACC_ALL_TIERS, tier 5 (the legacy layout, no g_total) among them
    tiers = re.search(r"#define DACC_KERNEL_TIERS\(X\)((?: X\(\d+\))+)", open(os.path.join(_CSRC, "tier_pipeline.hpp")).read()).group(1)
    assert sorted(int(l.split()[1]) for l in exp if l) == sorted([int(t) for t in re.findall(r"\d+", tiers)] + [5])
    assert len(got) == len(exp), "%d lines, the golden has %d" % (len(got), len(exp))
    for g, e in zip(got, exp):
        assert g == e

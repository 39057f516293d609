"""ctypes wrapper of the wavefront primitive probe (tests/waveprobe/): TEST HARNESS ONLY.
Two builds of the same probe bodies (tests/waveprobe/probe_body.hpp, which call daccord_amd/csrc/wave.hpp one primitive at a time):
libwaveprobe_host.so, the 64-lane host wavefront of wave_emul64.hpp under g++, and -- where hipcc exists -- libwaveprobe_dev.so, gfx950
kernels compiled with the product's flags (device code at -Os, max-ILP scheduler), i.e. the device branch of wave.hpp itself."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
sys.path.insert(0, _ROOT)
from daccord_amd.build import HIPCC_FLAGS  # noqa: E402

_DIR = os.path.join(_HERE, "waveprobe")
_SO_HOST = os.path.join(_DIR, "libwaveprobe_host.so")
_SO_DEV = os.path.join(_DIR, "libwaveprobe_dev.so")
_SRCS = [os.path.join(_DIR, f) for f in ("probe_body.hpp", "probe_api.h", "probe.hip", "probe_host.cpp")] + \
        [os.path.join(_ROOT, "daccord_amd", "csrc", f) for f in ("wave.hpp", "wave_emul64.hpp")]

JOB = np.dtype([("mode", "<u4"), ("n", "<u4"), ("off", "<u4"), ("pad", "<u4")])
IDXJOB = np.dtype([("p2", "<u4"), ("nk", "<u4"), ("koff", "<u4"), ("ioff", "<u4")])
SPACE_LDS, SPACE_GLOBAL = 0, 1
# field order of the outputs (tests/waveprobe/probe_body.hpp)
F32 = ("scan_pre", "scan_tot", "sum", "max", "or", "flag_pre", "flag_tot", "ballot", "any", "lanemask_lt")
F64 = ("sum64", "max64", "min64", "or64", "uni64")
FX = ("bcast", "bcast64", "uni", "shfl", "shfl64")


def _hipcc():
    h = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return h if os.path.exists(h) else None


def _stale(so):
    return not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in _SRCS)


def build(force=False):
    """libwaveprobe_host.so with g++; libwaveprobe_dev.so with hipcc for gfx950 where there is one (no GPU needed to compile)."""
    if force or _stale(_SO_HOST):
        subprocess.check_call(["g++", "-O2", "-w", "-std=c++17", "-fPIC", "-shared", "-DDACC_EMUL", "-DDACC_EMUL_LANES=64", "-DDACC_EMUL_IMPL",
                               "-o", _SO_HOST, os.path.join(_DIR, "probe_host.cpp")])
    hipcc = _hipcc()
    if hipcc and (force or _stale(_SO_DEV)):
        subprocess.check_call([hipcc] + HIPCC_FLAGS + ["-o", _SO_DEV, os.path.join(_DIR, "probe.hip")])
    return _SO_HOST


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class ProbeError(RuntimeError):
    pass


_libs = {}
_failed = {}


def _lib(kind):
    if kind not in _libs:
        so = _SO_DEV if kind == "dev" else _SO_HOST
        if kind == "host" or _hipcc():
            build()
        if not os.path.exists(so):
            raise ImportError("%s is not built: run `python -c 'import __graft_entry__ as g; g.build()'` where hipcc exists" % os.path.basename(so))
        L = C.CDLL(so)
        vp = C.c_void_p
        L.wp_error_string.restype = C.c_char_p; L.wp_error_string.argtypes = [C.c_int]
        L.wp_sort_pairs.argtypes = [vp, vp, C.c_uint32]
        L.wp_u32.argtypes = [vp, vp, vp, C.c_uint32]
        L.wp_u64.argtypes = [vp, vp, C.c_uint32]
        L.wp_xlane.argtypes = [vp, vp, vp, vp, vp, C.c_uint32]
        L.wp_sort.argtypes = [C.c_int, vp, C.c_uint32, vp, C.c_uint64]
        L.wp_sort_idx.argtypes = [C.c_int, vp, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64]
        L.wp_atomic.argtypes = [C.c_uint32, vp]
        assert L.wp_is_device() == (1 if kind == "dev" else 0)
        _libs[kind] = L
    return _libs[kind]


class Probe:
    """kind: "host" (64-lane host wavefront) or "dev" (gfx950 kernels).  A non-zero status of an entry point raises ProbeError with
    the library's text for it; nothing is tried twice."""

    def __init__(self, kind):
        self.kind = kind
        self._L = _lib(kind)

    @property
    def L(self):
        if self.kind in _failed:
            raise ProbeError("not run: an earlier entry point failed (%s)" % _failed[self.kind])
        return self._L

    def _chk(self, what, rc):
        if rc and rc != 1 and self.kind == "dev":
            _failed[self.kind] = "%s returned %d" % (what, rc)      # a HIP error: no further launch of this process reaches the device
        if rc:
            raise ProbeError("%s (%s probe): status %d: %s" % (what, self.kind, rc, (self._L.wp_error_string(rc) or b"").decode()))

    def sort_pairs(self):
        """[(CAP, R32)] of sort modes 0 .. n-1: the instantiations of wv_sort_keys compiled into the probe"""
        cap = np.zeros(64, np.uint32); r32 = np.zeros(64, np.int32)
        n = self.L.wp_sort_pairs(_ptr(cap), _ptr(r32), 64)
        return [(int(cap[i]), bool(r32[i])) for i in range(n)]

    def u32(self, vals, flags):
        vals = np.ascontiguousarray(vals, np.uint32); flags = np.ascontiguousarray(flags, np.uint32)
        assert vals.shape == flags.shape and vals.shape[1] == 64
        out = np.zeros((len(vals), len(F32), 64), np.uint64)
        self._chk("wp_u32", self.L.wp_u32(_ptr(vals), _ptr(flags), _ptr(out), len(vals)))
        return out

    def u64(self, vals):
        vals = np.ascontiguousarray(vals, np.uint64)
        assert vals.shape[1] == 64
        out = np.zeros((len(vals), len(F64), 64), np.uint64)
        self._chk("wp_u64", self.L.wp_u64(_ptr(vals), _ptr(out), len(vals)))
        return out

    def xlane(self, v32, v64, src, bsrc):
        v32 = np.ascontiguousarray(v32, np.uint32); v64 = np.ascontiguousarray(v64, np.uint64)
        src = np.ascontiguousarray(src, np.int32); bsrc = np.ascontiguousarray(bsrc, np.int32)
        assert v32.shape == v64.shape == src.shape and v32.shape[1] == 64 and bsrc.shape == (len(v32),)
        out = np.zeros((len(v32), len(FX), 64), np.uint64)
        self._chk("wp_xlane", self.L.wp_xlane(_ptr(v32), _ptr(v64), _ptr(src), _ptr(bsrc), _ptr(out), len(v32)))
        return out

    def sort(self, space, jobs, keys):
        """the key buffer after every job sorted its slice in place (the slices must not overlap)"""
        jobs = np.ascontiguousarray(jobs, JOB); keys = np.array(keys, np.uint64, copy=True)
        self._chk("wp_sort", self.L.wp_sort(space, _ptr(jobs), len(jobs), _ptr(keys), len(keys)))
        return keys

    def sort_idx(self, space, jobs, kbuf, idx):
        jobs = np.ascontiguousarray(jobs, IDXJOB); kbuf = np.ascontiguousarray(kbuf, np.uint64); idx = np.array(idx, np.uint32, copy=True)
        self._chk("wp_sort_idx", self.L.wp_sort_idx(space, _ptr(jobs), len(jobs), _ptr(kbuf), len(kbuf), _ptr(idx), len(idx)))
        return idx

    def atomic(self, init):
        out = np.zeros((3, 65), np.uint32)
        self._chk("wp_atomic", self.L.wp_atomic(init, _ptr(out)))
        return out

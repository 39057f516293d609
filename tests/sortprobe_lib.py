"""ctypes wrapper of the sort probe (tests/sortprobe/sortprobe.cpp): TEST HARNESS ONLY, host code compiled on demand with g++.
The engines' replays of libstdc++'s std::sort on the reverse paths of a window, run on caller-supplied (front, baselen) keys."""
import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SRC = os.path.join(_HERE, "sortprobe", "sortprobe.cpp")
_SO = os.path.join(_HERE, "sortprobe", "libsortprobe.so")
_DEPS = [_SRC] + [os.path.join(_ROOT, "daccord_amd", "csrc", f) for f in os.listdir(os.path.join(_ROOT, "daccord_amd", "csrc")) if f.endswith(".hpp")]

GENERIC, TIER3, TIER3_KEYED, TIER1, TIER1_KEYED = range(5)
TIERS = (TIER3, TIER3_KEYED, TIER1, TIER1_KEYED)
REFUSED = 1024      # a tier's flag for "introsort's depth limit reached, not reproduced here"


def build(force=False):
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(s) for s in _DEPS):
        subprocess.check_call(["g++", "-O2", "-w", "-std=c++17", "-fPIC", "-pthread", "-ffp-contract=off", "-shared", "-o", _SO, _SRC])
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_SO)
        vp = C.c_void_p
        L.sp_capacity.restype = C.c_uint32; L.sp_capacity.argtypes = [C.c_int]
        L.sp_sort.argtypes = [C.c_int, vp, vp, C.c_uint32, vp, vp, vp]
        L.sp_expected.argtypes = [vp, vp, C.c_uint32, vp]
        L.sp_killer.argtypes = [C.c_uint32, C.c_int, C.c_uint32, vp]
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def capacity(engine):
    return int(lib().sp_capacity(engine))


def sort(engine, front, baselen):
    """(permutation, overflow flags, heapsort fallbacks taken) of an engine's sort"""
    front = np.ascontiguousarray(front, np.uint32); baselen = np.ascontiguousarray(baselen, np.uint16)
    assert front.shape == baselen.shape
    perm = np.full(len(front) + 1, -1, np.int32); flags = C.c_uint32(); fb = C.c_int32()
    rc = lib().sp_sort(engine, _ptr(front), _ptr(baselen), len(front), _ptr(perm), C.byref(flags), C.byref(fb))
    if rc:
        raise ValueError("sp_sort: status %d (2: more keys than the engine holds, 3: base length above 255, 4: too many distinct fronts)" % rc)
    assert perm[-1] == -1
    return perm[:-1], int(flags.value), int(fb.value)


def expected(front, baselen):
    """std::sort over an array of (front, baselen, index) structs with the engines' comparator"""
    front = np.ascontiguousarray(front, np.uint32); baselen = np.ascontiguousarray(baselen, np.uint16)
    perm = np.full(len(front) + 1, -1, np.int32)
    lib().sp_expected(_ptr(front), _ptr(baselen), len(front), _ptr(perm))
    return perm[:-1]


def killer(n, mirror=False, copies=1):
    """keys 0 .. (n-1) // copies of a median-of-3 killer sequence for this libstdc++'s std::sort (McIlroy's adversary, answering with `copies`
    equal keys per value); mirror: pivots at the high end"""
    rank = np.zeros(n + 1, np.uint32)
    assert lib().sp_killer(n, 1 if mirror else 0, copies, _ptr(rank)) == 0
    return rank[:-1] // copies

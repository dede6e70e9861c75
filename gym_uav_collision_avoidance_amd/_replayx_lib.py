"""ctypes binding of libuavx_replayx.so: the n-step replay sampler with recency-weighted draws (include/uavx_nstep.h,
DESIGN.md §22).  One unit, described once in UNIT -- header, bound ABI version, every exported function with its restype
and argtypes, the version function first.  Built, checked for staleness and loaded like the other two libraries
(_native.py), from a directory of its own: libuavx_actor.so and libuavx.so, their file lists and the source hashes that
tests and profiles pin do not change with it.  The ring is _actor_lib.ReplayRing and the status codes are _actor_lib's.
There is NO fallback: a missing library or device raises."""
import ctypes
import os

from . import _actor_lib, _native
from ._actor_lib import ERR_INVALID_ARG, OK, ReplayRing, Unit  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
CSRC = os.path.join(_HERE, "replay_csrc")
LIB_PATH = os.path.join(CSRC, "libuavx_replayx.so")

NSTEP_MAX = 8                   # UAVX_NSTEP_MAX
NSTEP_MAX_ROWS = 1048576        # UAVX_NSTEP_MAX_ROWS
NSTEP_SINGLE_ROWS = 1024        # UAVX_NSTEP_SINGLE_ROWS: up to here one launch and no workspace

_lib_handle = None


class NStepArgs(ctypes.Structure):
    """uavx_nstep_args of include/uavx_nstep.h."""
    _fields_ = [("ring", ctypes.POINTER(ReplayRing)), ("count", ctypes.c_int64), ("count_dev", ctypes.c_void_p),
                ("u", ctypes.c_void_p), ("u_cols", ctypes.c_int32), ("n_step", ctypes.c_int32), ("gamma", ctypes.c_double),
                ("recency", ctypes.c_float), ("rows", ctypes.c_int64), ("state", ctypes.c_void_p),
                ("action", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("next_state", ctypes.c_void_p),
                ("mask", ctypes.c_void_p), ("length", ctypes.c_void_p), ("truncated", ctypes.c_void_p),
                ("ended", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64)]


_vp, _i64, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int

UNIT = Unit("n-step replay", os.path.join(_INCLUDE, "uavx_nstep.h"), "uavx_nstep_version", 1, {
    "uavx_nstep_version": (_i32, []),
    "uavx_nstep_workspace_bytes": (_i32, [_i64, ctypes.POINTER(_i64)]),
    "uavx_nstep_sample": (_i32, [ctypes.POINTER(NStepArgs), _vp])})
HEADER, SYMBOLS, ABI_VERSION = UNIT.header, tuple(UNIT.functions), UNIT.abi


def _sources():
    # the two headers uavx_nstep.h includes decide the struct layouts and status codes as much as it does
    return [os.path.join(CSRC, "uavx_nstep.hip"), HEADER, _actor_lib.REPLAY_HEADER, _actor_lib.HEADER]


def source_hash():
    """sha256 over the code (comments and whitespace dropped) of replay_csrc/uavx_nstep.hip, include/uavx_nstep.h and the two
    headers it includes, plus the Makefile without comments and any HIPCC / ARCH / HIPFLAGS override; 16 hex digits."""
    return _native.source_hash(CSRC, _sources())


def build(force=False):
    """hipcc build of replay_csrc/ into libuavx_replayx.so (gfx950), under a file lock and renamed into place."""
    return _native.build(CSRC, LIB_PATH, source_hash, _up_to_date, force)


def _up_to_date():
    """Does LIB_PATH carry the hash of the sources in the tree (read from the file, not through dlopen)?"""
    return _native.up_to_date(CSRC, LIB_PATH, b"UAVX_REPLAYX_SRC_HASH", _sources(), source_hash)


def load():
    global _lib_handle
    if _lib_handle is not None:
        return _lib_handle
    if not os.path.exists(LIB_PATH) or not _up_to_date():
        build()                 # a build, not a fallback: a compile error is raised as such
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in UNIT.functions.items():            # the version function comes first
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
        if name == UNIT.version and f() != UNIT.abi:
            raise RuntimeError(f"{LIB_PATH} speaks {UNIT.word} ABI version {f()}, this package binds {UNIT.abi}: "
                               f"rebuild it (`make -B -C {CSRC}`)")
    _lib_handle = L
    return L


def check(rc, what):
    """The status codes and their texts are uavx_actor.h's."""
    _actor_lib.check(rc, what)

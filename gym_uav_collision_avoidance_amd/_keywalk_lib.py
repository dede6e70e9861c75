"""ctypes binding of libuavx_keywalk.so: the n-step walk from the keys of a prioritized sample (include/uavx_keywalk.h,
DESIGN.md §25).  Built, checked for staleness and loaded like libuavx_prio.so (_prio_lib.py, on _native.py), from a
directory of its own so that the actor and prio libraries and the source hashes they carry do not change with it.  One
unit: its header, the ABI version this package binds and every exported function with its restype and argtypes.  There is
NO fallback: a missing library or device raises."""
import ctypes
import glob
import os

from . import _native
from ._actor_lib import ERR_INVALID_ARG, OK, ReplayRing  # noqa: F401  (the ring and the status codes are uavx_replay.h's)

_HERE = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
CSRC = os.path.join(_HERE, "keywalk_csrc")
LIB_PATH = os.path.join(CSRC, "libuavx_keywalk.so")
HEADER = os.path.join(_INCLUDE, "uavx_keywalk.h")
ABI_VERSION = 1

MAX_STEP = 8                    # UAVX_KEYWALK_MAX_STEP
MAX_ROWS = 1048576              # UAVX_KEYWALK_MAX_ROWS

_lib_handle = None


class Args(ctypes.Structure):
    """uavx_keywalk_args of include/uavx_keywalk.h."""
    _fields_ = [("ring", ctypes.POINTER(ReplayRing)), ("count", ctypes.c_int64), ("count_dev", ctypes.c_void_p),
                ("key", ctypes.c_void_p), ("rows", ctypes.c_int64), ("n_step", ctypes.c_int32), ("gamma", ctypes.c_double),
                ("reward", ctypes.c_void_p), ("next_state", ctypes.c_void_p), ("mask", ctypes.c_void_p),
                ("length", ctypes.c_void_p), ("truncated", ctypes.c_void_p), ("ended", ctypes.c_void_p)]


# every symbol the header declares (tests check the built library exports exactly these) -> (restype, argtypes); the version
# function comes first
FUNCTIONS = {
    "uavx_keywalk_version": (ctypes.c_int, []),
    "uavx_keywalk": (ctypes.c_int, [ctypes.POINTER(Args), ctypes.c_void_p]),
}
SYMBOLS = tuple(FUNCTIONS)


def _sources():
    return (sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
            + [HEADER, os.path.join(_INCLUDE, "uavx_replay.h"), os.path.join(_INCLUDE, "uavx_actor.h")])


def source_hash():
    """sha256 over the code of keywalk_csrc/*.hip and the three headers it includes, plus the Makefile without comments and
    any HIPCC / ARCH / HIPFLAGS override (_native.source_hash); 16 hex digits."""
    return _native.source_hash(CSRC, _sources())


def build(force=False):
    """hipcc build of keywalk_csrc/ into libuavx_keywalk.so (gfx950), under a file lock and renamed into place
    (_native.build)."""
    return _native.build(CSRC, LIB_PATH, source_hash, _up_to_date, force)


def _up_to_date():
    """Does LIB_PATH carry the hash of the sources in the tree (read from the file, not through dlopen)?"""
    return _native.up_to_date(CSRC, LIB_PATH, b"UAVX_KEYWALK_SRC_HASH", _sources(), source_hash)


def load():
    global _lib_handle
    if _lib_handle is not None:
        return _lib_handle
    if not os.path.exists(LIB_PATH) or not _up_to_date():
        build()                 # a build, not a fallback: a compile error is raised as such
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in FUNCTIONS.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    if L.uavx_keywalk_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks key-walk ABI version {L.uavx_keywalk_version()}, this package binds "
                           f"{ABI_VERSION}: rebuild it (`make -B -C {CSRC}`)")
    _lib_handle = L
    return L


_ERRORS = {-1: "invalid argument", -2: "HIP error", -3: "unsupported", -4: "not packed"}


def check(rc, what):
    if rc != OK:
        raise RuntimeError(f"uavx: {what} failed: {_ERRORS.get(rc, 'unknown error')} ({rc})")

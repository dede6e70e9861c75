"""ctypes binding of libuavx_prio.so: the prioritized-replay kernels (include/uavx_prio.h).  Built, checked
for staleness and loaded like libuavx_actor.so (_actor_lib.py, on _native.py), from a directory of its own so that the actor
library and the source hash it carries do not change with it.  One unit: its header, the ABI version this package binds and
every exported function with its restype and argtypes.  There is NO fallback: a missing library or device raises."""
import ctypes
import glob
import os

from . import _native
from ._actor_lib import ERR_INVALID_ARG, OK, ReplayRing  # noqa: F401  (the ring and the status codes are uavx_replay.h's)

_HERE = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
CSRC = os.path.join(_HERE, "prio_csrc")
LIB_PATH = os.path.join(CSRC, "libuavx_prio.so")
HEADER = os.path.join(_INCLUDE, "uavx_prio.h")
ABI_VERSION = 1

ONE = 65536                     # UAVX_PRIO_ONE: Q16.16
MAX_ENTRIES = 67108864          # UAVX_PRIO_MAX_ENTRIES
MAX_ROWS = 1048576              # UAVX_PRIO_MAX_ROWS
MAX_TOWERS = 2                  # UAVX_PRIO_MAX_TOWERS
FAN = 64                        # children per node of the partial sums
RECORD_BYTES = 32               # sizeof(uavx_prio_record)

_lib_handle = None


class Record(ctypes.Structure):
    """uavx_prio_record of include/uavx_prio.h."""
    _fields_ = [("total", ctypes.c_uint64), ("p_min", ctypes.c_uint32), ("p_max", ctypes.c_uint32),
                ("seen", ctypes.c_int64), ("valid", ctypes.c_uint64)]


class State(ctypes.Structure):
    """uavx_prio_state of include/uavx_prio.h."""
    _fields_ = [("ring", ctypes.POINTER(ReplayRing)), ("count", ctypes.c_int64), ("count_dev", ctypes.c_void_p),
                ("table", ctypes.c_void_p), ("sums", ctypes.c_void_p), ("sums_bytes", ctypes.c_int64),
                ("rec", ctypes.c_void_p)]


class SampleArgs(ctypes.Structure):
    """uavx_prio_sample_args of include/uavx_prio.h."""
    _fields_ = [("u", ctypes.c_void_p), ("rows", ctypes.c_int64), ("stratified", ctypes.c_int32), ("beta", ctypes.c_float),
                ("beta_dev", ctypes.c_void_p), ("state", ctypes.c_void_p), ("action", ctypes.c_void_p),
                ("reward", ctypes.c_void_p), ("next_state", ctypes.c_void_p), ("mask", ctypes.c_void_p),
                ("truncated", ctypes.c_void_p), ("ended", ctypes.c_void_p), ("key", ctypes.c_void_p),
                ("weight", ctypes.c_void_p)]


_vp, _i64, _i32, _f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
_pstate = ctypes.POINTER(State)

# every symbol the header declares (tests check the built library exports each of them) -> (restype, argtypes); the version
# function comes first
FUNCTIONS = {
    "uavx_prio_version": (_i32, []),
    "uavx_prio_state_bytes": (_i32, [_i64, ctypes.POINTER(_i64)]),
    "uavx_prio_refresh": (_i32, [_pstate, _vp]),
    "uavx_prio_sample": (_i32, [_pstate, ctypes.POINTER(SampleArgs), _vp]),
    "uavx_prio_update": (_i32, [_pstate, _vp, _vp, _i32, _vp, _i64, _i64, _f64, _f64, _vp]),
}
SYMBOLS = tuple(FUNCTIONS)


def _sources():
    return (sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
            + [HEADER, os.path.join(_INCLUDE, "uavx_replay.h"), os.path.join(_INCLUDE, "uavx_actor.h")])


def source_hash():
    """sha256 over the code of prio_csrc/*.hip and the three headers it includes, plus the Makefile without comments and any
    HIPCC / ARCH / HIPFLAGS override (_native.source_hash); 16 hex digits."""
    return _native.source_hash(CSRC, _sources())


def build(force=False):
    """hipcc build of prio_csrc/ into libuavx_prio.so (gfx950), under a file lock and renamed into place (_native.build)."""
    return _native.build(CSRC, LIB_PATH, source_hash, _up_to_date, force)


def _up_to_date():
    """Does LIB_PATH carry the hash of the sources in the tree (read from the file, not through dlopen)?"""
    return _native.up_to_date(CSRC, LIB_PATH, b"UAVX_PRIO_SRC_HASH", _sources(), source_hash)


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
    if L.uavx_prio_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks prioritized-replay ABI version {L.uavx_prio_version()}, this package binds "
                           f"{ABI_VERSION}: rebuild it (`make -B -C {CSRC}`)")
    _lib_handle = L
    return L


_ERRORS = {-1: "invalid argument", -2: "HIP error", -3: "unsupported", -4: "not packed"}


def check(rc, what):
    if rc != OK:
        raise RuntimeError(f"uavx: {what} failed: {_ERRORS.get(rc, 'unknown error')} ({rc})")

"""ctypes binding of libuavx_gae.so: GAE(λ) advantages and returns over the device ring and their normalisation
(include/uavx_gae.h).  Built, checked for staleness and loaded like libuavx_clip.so (_clip_lib.py, on
_native.py), from a directory of its own so that no other library and no source hash changes with it.  One unit: its header,
the ABI version this package binds and every exported function with its restype and argtypes.  Nothing imports this module
until a RolloutAdvantages computes.  There is NO fallback: a missing library or device raises."""
import ctypes
import glob
import os

from . import _native
from ._actor_lib import ERR_HIP, ERR_INVALID_ARG, OK  # noqa: F401  (the status codes are uavx_actor.h's)

_HERE = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
CSRC = os.path.join(_HERE, "gae_csrc")
LIB_PATH = os.path.join(CSRC, "libuavx_gae.so")
HEADER = os.path.join(_INCLUDE, "uavx_gae.h")
ABI_VERSION = 1

BLOCK = 256                     # UAVX_GAE_BLOCK
STATS_BYTES = 24

_lib_handle = None

_vp, _i64, _f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double


class Ring(ctypes.Structure):
    """uavx_gae_ring of include/uavx_gae.h."""
    _fields_ = [("rew", _vp), ("done", _vp), ("skip", _vp), ("ended", _vp), ("slots", _i64), ("envs", _i64),
                ("agents", _i64), ("learners", _i64)]


class Stats(ctypes.Structure):
    """uavx_gae_stats of include/uavx_gae.h (the layout of the device record; never filled on the host)."""
    _fields_ = [("n", _i64), ("mean", _f64), ("std", _f64)]


# every symbol the header declares (tests check the built library exports exactly these) -> (restype, argtypes); the version
# function comes first
FUNCTIONS = {
    "uavx_gae_version": (ctypes.c_int, []),
    "uavx_gae_workspace_bytes": (ctypes.c_int, [ctypes.POINTER(Ring), ctypes.POINTER(_i64)]),
    "uavx_gae_compute": (ctypes.c_int, [ctypes.POINTER(Ring), _vp, _i64, _i64, _f64, _f64, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _i64, _vp]),
}
SYMBOLS = tuple(FUNCTIONS)


def _sources():
    return (sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
            + [HEADER, os.path.join(_INCLUDE, "uavx_actor.h")])


def source_hash():
    """sha256 over the code of gae_csrc/*.hip and the two headers it includes, plus the Makefile without comments and any
    HIPCC / ARCH / HIPFLAGS override (_native.source_hash); 16 hex digits."""
    return _native.source_hash(CSRC, _sources())


def build(force=False):
    """hipcc build of gae_csrc/ into libuavx_gae.so (gfx950), under a file lock and renamed into place (_native.build)."""
    return _native.build(CSRC, LIB_PATH, source_hash, _up_to_date, force)


def _up_to_date():
    """Does LIB_PATH carry the hash of the sources in the tree (read from the file, not through dlopen)?"""
    return _native.up_to_date(CSRC, LIB_PATH, b"UAVX_GAE_SRC_HASH", _sources(), source_hash)


def loaded():
    """Has this process mapped the library?"""
    return _lib_handle is not None


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
    if L.uavx_gae_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks gae ABI version {L.uavx_gae_version()}, this package binds "
                           f"{ABI_VERSION}: rebuild it (`make -B -C {CSRC}`)")
    _lib_handle = L
    return L


_ERRORS = {-1: "invalid argument", -2: "HIP error", -3: "unsupported"}


def check(rc, what):
    if rc != OK:
        raise RuntimeError(f"uavx: {what} failed: {_ERRORS.get(rc, 'unknown error')} ({rc})")

"""ctypes binding of libuavx_ppo.so: PPO's sampling and loss heads (include/uavx_ppo.h).  Built, checked for
staleness and loaded like libuavx_gae.so (_gae_lib.py, on _native.py), from a directory of its own so that no other library
and no source hash changes with it.  One unit: its header, the ABI version this package binds and every exported function
with its restype and argtypes.  Nothing imports this module until a PPOHeads launches.  There is NO fallback: a missing
library or device raises."""
import ctypes
import glob
import os

from . import _native
from ._actor_lib import ERR_HIP, ERR_INVALID_ARG, OK  # noqa: F401  (the status codes are uavx_actor.h's)

_HERE = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
CSRC = os.path.join(_HERE, "ppo_csrc")
LIB_PATH = os.path.join(CSRC, "libuavx_ppo.so")
HEADER = os.path.join(_INCLUDE, "uavx_ppo.h")
ABI_VERSION = 1

BLOCK = 256                     # UAVX_PPO_BLOCK
PARTIAL_BYTES = 32              # workspace per workgroup: four float64

_lib_handle = None

_vp, _i64, _f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double

# every symbol the header declares (tests check the built library exports exactly these) -> (restype, argtypes); the version
# function comes first
FUNCTIONS = {
    "uavx_ppo_version": (ctypes.c_int, []),
    "uavx_ppo_sample": (ctypes.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "uavx_ppo_loss_workspace_bytes": (ctypes.c_int, [_i64, ctypes.POINTER(_i64)]),
    "uavx_ppo_loss": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _f64, _f64, _f64, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _i64, _vp]),
}
SYMBOLS = tuple(FUNCTIONS)


def _sources():
    return (sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
            + [HEADER, os.path.join(_INCLUDE, "uavx_actor.h")])


def source_hash():
    """sha256 over the code of ppo_csrc/*.hip and the two headers it includes, plus the Makefile without comments and any
    HIPCC / ARCH / HIPFLAGS override (_native.source_hash); 16 hex digits."""
    return _native.source_hash(CSRC, _sources())


def build(force=False):
    """hipcc build of ppo_csrc/ into libuavx_ppo.so (gfx950), under a file lock and renamed into place (_native.build)."""
    return _native.build(CSRC, LIB_PATH, source_hash, _up_to_date, force)


def _up_to_date():
    """Does LIB_PATH carry the hash of the sources in the tree (read from the file, not through dlopen)?"""
    return _native.up_to_date(CSRC, LIB_PATH, b"UAVX_PPO_SRC_HASH", _sources(), source_hash)


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
    if L.uavx_ppo_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks ppo ABI version {L.uavx_ppo_version()}, this package binds "
                           f"{ABI_VERSION}: rebuild it (`make -B -C {CSRC}`)")
    _lib_handle = L
    return L


_ERRORS = {-1: "invalid argument", -2: "HIP error", -3: "unsupported"}


def check(rc, what):
    if rc != OK:
        raise RuntimeError(f"uavx: {what} failed: {_ERRORS.get(rc, 'unknown error')} ({rc})")

"""ctypes binding of libuavx_wgrad.so: the weighted critic-loss gradient (include/uavx_wcritic_grad.h).
Built, checked for staleness and loaded like libuavx_prio.so (_prio_lib.py, on _native.py), from a directory of its own so
that the actor library and the source hash it carries do not change with it.  The library compiles two files of
actor_csrc/ as they stand (uavx_grad_impl.hpp and the dW2 weights kernel of uavx_grad_common.hip), so its own source hash
covers them too.  One unit: its header, the ABI version this package binds and every exported function with its restype and
argtypes.  There is NO fallback: a missing library or device raises."""
import ctypes
import glob
import os

from . import _native
from ._actor_lib import DDPG, ERR_HIP, ERR_INVALID_ARG, ERR_UNSUPPORTED, GRAD_L1, GRAD_MSE, OK, SAC, TD3  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
_ACTOR_CSRC = os.path.join(_HERE, "actor_csrc")
CSRC = os.path.join(_HERE, "wgrad_csrc")
LIB_PATH = os.path.join(CSRC, "libuavx_wgrad.so")
HEADER = os.path.join(_INCLUDE, "uavx_wcritic_grad.h")
ABI_VERSION = 1

MAX_ROWS = 262144               # UAVX_WCRITIC_GRAD_MAX_ROWS

# what the library compiles from actor_csrc/, and the headers those files include
SHARED = tuple(os.path.join(_ACTOR_CSRC, f) for f in ("uavx_grad_common.hip", "uavx_grad_impl.hpp", "uavx_actor_impl.hpp"))
SHARED_HEADERS = tuple(os.path.join(_INCLUDE, f) for f in ("uavx_actor.h", "uavx_critic.h"))

_lib_handle = None

_vp, _i64, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
_pvp = ctypes.POINTER(_vp)

# every symbol the header declares (tests check the built library exports each of them) -> (restype, argtypes); the version
# function comes first
FUNCTIONS = {
    "uavx_wcritic_grad_version": (_i32, []),
    "uavx_wcritic_grad_workspace_bytes": (_i32, [_i32, _i32, _i32, _i32, _i64, ctypes.POINTER(_i64)]),
    "uavx_wcritic_grad": (_i32, [_i32, _i32, _i32, _i32, _i32, _pvp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _pvp,
                                 _vp, _vp, _vp, _i64, _vp]),
}
SYMBOLS = tuple(FUNCTIONS)


def _sources():
    return (sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
            + [HEADER] + list(SHARED) + list(SHARED_HEADERS))


def source_hash():
    """sha256 over the code of wgrad_csrc/*.hip, its header, the three files of actor_csrc/ it compiles and the two headers
    those include, plus the Makefile without comments and any HIPCC / ARCH / HIPFLAGS override (_native.source_hash); 16
    hex digits."""
    return _native.source_hash(CSRC, _sources())


def build(force=False):
    """hipcc build of wgrad_csrc/ into libuavx_wgrad.so (gfx950), under a file lock and renamed into place (_native.build)."""
    return _native.build(CSRC, LIB_PATH, source_hash, _up_to_date, force)


def _up_to_date():
    """Does LIB_PATH carry the hash of the sources in the tree (read from the file, not through dlopen)?"""
    return _native.up_to_date(CSRC, LIB_PATH, b"UAVX_WGRAD_SRC_HASH", _sources(), source_hash)


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
    if L.uavx_wcritic_grad_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks weighted-critic-gradient ABI version {L.uavx_wcritic_grad_version()}, this "
                           f"package binds {ABI_VERSION}: rebuild it (`make -B -C {CSRC}`)")
    _lib_handle = L
    return L


_ERRORS = {-1: "invalid argument", -2: "HIP error", -3: "unsupported"}


def check(rc, what):
    if rc != OK:
        raise RuntimeError(f"uavx: {what} failed: {_ERRORS.get(rc, 'unknown error')} ({rc})")

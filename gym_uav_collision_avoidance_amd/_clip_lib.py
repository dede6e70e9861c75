"""ctypes binding of libuavx_clip.so: the Adam step behind a clip of the global gradient norm (include/uavx_clip.h,
DESIGN.md §26).  Built, checked for staleness and loaded like libuavx_prio.so (_prio_lib.py, on _native.py), from a
directory of its own so that the actor library and the source hash it carries do not change with it.  One unit: its header,
the ABI version this package binds and every exported function with its restype and argtypes.  Nothing imports this module
until a FusedAdam is built with max_grad_norm.  There is NO fallback: a missing library or device raises."""
import ctypes
import glob
import os

from . import _native
from ._actor_lib import ERR_HIP, ERR_INVALID_ARG, OK  # noqa: F401  (the status codes are uavx_actor.h's)

_HERE = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
CSRC = os.path.join(_HERE, "clip_csrc")
LIB_PATH = os.path.join(CSRC, "libuavx_clip.so")
HEADER = os.path.join(_INCLUDE, "uavx_clip.h")
ABI_VERSION = 1

MAX_TENSORS = 16                # UAVX_CLIP_MAX_TENSORS
MAX_GROUPS = 16                 # UAVX_CLIP_MAX_GROUPS
BLOCK = 1024                    # UAVX_CLIP_BLOCK
RECORD_BYTES = 16

_lib_handle = None

_vp, _i64, _i32, _f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double


class Record(ctypes.Structure):
    """uavx_clip_record of include/uavx_clip.h (the layout of the device record; never filled on the host)."""
    _fields_ = [("norm", ctypes.c_float), ("coef", ctypes.c_float), ("clipped", _i64)]


class Group(ctypes.Structure):
    """uavx_clip_group of include/uavx_clip.h."""
    _fields_ = [("n", _i32), ("params", _vp), ("grads", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("max_exp_avg_sq", _vp),
                ("targets", _vp), ("numel", _vp), ("lr", _f64), ("beta1", _f64), ("beta2", _f64), ("eps", _f64), ("tau", _f64),
                ("step", _vp), ("scalars", _vp)]


# every symbol the header declares (tests check the built library exports exactly these) -> (restype, argtypes); the version
# function comes first
FUNCTIONS = {
    "uavx_clip_version": (ctypes.c_int, []),
    "uavx_clip_workspace_bytes": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(Group), ctypes.POINTER(_i64)]),
    "uavx_clip_step": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(Group), _vp, _i64, _vp, _vp, _vp]),
}
SYMBOLS = tuple(FUNCTIONS)


def _sources():
    return (sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
            + [HEADER, os.path.join(_INCLUDE, "uavx_actor.h")])


def source_hash():
    """sha256 over the code of clip_csrc/*.hip and the two headers it includes, plus the Makefile without comments and any
    HIPCC / ARCH / HIPFLAGS override (_native.source_hash); 16 hex digits."""
    return _native.source_hash(CSRC, _sources())


def build(force=False):
    """hipcc build of clip_csrc/ into libuavx_clip.so (gfx950), under a file lock and renamed into place (_native.build)."""
    return _native.build(CSRC, LIB_PATH, source_hash, _up_to_date, force)


def _up_to_date():
    """Does LIB_PATH carry the hash of the sources in the tree (read from the file, not through dlopen)?"""
    return _native.up_to_date(CSRC, LIB_PATH, b"UAVX_CLIP_SRC_HASH", _sources(), source_hash)


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
    if L.uavx_clip_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks clip ABI version {L.uavx_clip_version()}, this package binds "
                           f"{ABI_VERSION}: rebuild it (`make -B -C {CSRC}`)")
    _lib_handle = L
    return L


_ERRORS = {-1: "invalid argument", -2: "HIP error", -3: "unsupported"}


def check(rc, what):
    if rc != OK:
        raise RuntimeError(f"uavx: {what} failed: {_ERRORS.get(rc, 'unknown error')} ({rc})")

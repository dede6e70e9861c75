"""libuavx_clip.so: the Adam step behind a clip of the norm of all gradients (include/uavx_clip.h), declared
once: the constants and structures of its header, its one unit -- header, bound ABI version, every exported function with
its restype and argtypes -- and LIB = _native.Library(...) over it, which is sources, hash, build, staleness, load and bind.
The module's other names are aliases of that object and of the table.  Its directory is its own; the clip, gae, ppo and norm
libraries share the headers of common_csrc/, whose code enters the source hash of each of the four; of those headers the actor,
prio and keywalk libraries use uavx_entry.hpp alone, and the env library none (the actor library's Adam unit, whose arithmetic
this one restates, stays as it is).
Nothing imports this module until a FusedAdam is built with max_grad_norm, and importing it neither builds nor maps anything.
There is NO fallback: a missing library or device raises."""
import ctypes

from . import _native
from ._actor_lib import ERR_HIP, ERR_INVALID_ARG, OK  # noqa: F401  (the status codes are uavx_actor.h's)

MAX_TENSORS = 16                # UAVX_CLIP_MAX_TENSORS
MAX_GROUPS = 16                 # UAVX_CLIP_MAX_GROUPS
BLOCK = 1024                    # UAVX_CLIP_BLOCK
RECORD_BYTES = 16

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
ABI_VERSION = 1

LIB = _native.Library("clip_csrc", "libuavx_clip.so", b"UAVX_CLIP_SRC_HASH",
                      [_native.unit("clip", "uavx_clip.h", ABI_VERSION, FUNCTIONS)], extras=("uavx_actor.h",),
                      shared=("uavx_block_reduce.hpp", "uavx_entry.hpp"))
CSRC, LIB_PATH, HEADER = LIB.csrc, LIB.path, LIB.units[0].header
load, loaded, build, source_hash, _sources, _up_to_date, check = (LIB.load, LIB.loaded, LIB.build, LIB.source_hash,
                                                                  LIB.sources, LIB.up_to_date, LIB.check)

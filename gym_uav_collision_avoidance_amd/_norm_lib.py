"""libuavx_norm.so: running observation and return statistics over the device ring and the two calls that apply them
(include/uavx_norm.h), declared once: the constants and structures of its header, its one unit -- header, bound
ABI version, every exported function with its restype and argtypes -- and LIB = _native.Library(...) over it, which is
sources, hash, build, staleness, load and bind.  The module's other names are aliases of that object and of the table.  Its
directory is its own; the clip, gae, ppo and norm libraries share the headers of common_csrc/, whose code enters the source
hash of each of the four; of those headers the actor, prio and keywalk libraries use uavx_entry.hpp alone, and the env library none.  Nothing imports this module until a
RolloutNormalizer folds or applies, and importing it neither builds nor maps anything.  There is NO fallback: a missing library
or device raises."""
import ctypes

from . import _native
from ._actor_lib import ERR_HIP, ERR_INVALID_ARG, OK  # noqa: F401  (the status codes are uavx_actor.h's)

BLOCK = 256                     # UAVX_NORM_BLOCK
MAX_FEATURES = 16               # UAVX_NORM_MAX_FEATURES
RECORD_BYTES = 288

_vp, _i64, _f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double


class Ring(ctypes.Structure):
    """uavx_norm_ring of include/uavx_norm.h."""
    _fields_ = [("rew", _vp), ("done", _vp), ("skip", _vp), ("ended", _vp), ("slots", _i64), ("envs", _i64),
                ("agents", _i64), ("learners", _i64)]


class Record(ctypes.Structure):
    """uavx_norm_record of include/uavx_norm.h (the layout of the device record; never filled on the host)."""
    _fields_ = [("n_obs", _i64), ("mean", _f64 * MAX_FEATURES), ("M2", _f64 * MAX_FEATURES), ("n_ret", _i64),
                ("mean_ret", _f64), ("M2_ret", _f64)]


# every symbol the header declares (tests check the built library exports exactly these) -> (restype, argtypes); the version
# function comes first
FUNCTIONS = {
    "uavx_norm_version": (ctypes.c_int, []),
    "uavx_norm_workspace_bytes": (ctypes.c_int, [ctypes.POINTER(Ring), _i64, ctypes.POINTER(_i64)]),
    "uavx_norm_fold_obs": (ctypes.c_int, [ctypes.POINTER(Ring), _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp]),
    "uavx_norm_fold_returns": (ctypes.c_int, [ctypes.POINTER(Ring), _i64, _i64, _f64, _vp, _vp, _vp, _i64, _vp]),
    "uavx_norm_apply_obs": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, _f64, _f64, _vp]),
    "uavx_norm_scale_rewards": (ctypes.c_int, [_vp, _vp, _vp, _i64, _f64, _f64, _vp]),
}
SYMBOLS = tuple(FUNCTIONS)
ABI_VERSION = 1

LIB = _native.Library("norm_csrc", "libuavx_norm.so", b"UAVX_NORM_SRC_HASH",
                      [_native.unit("norm", "uavx_norm.h", ABI_VERSION, FUNCTIONS)], extras=("uavx_actor.h",),
                      shared=("uavx_block_reduce.hpp", "uavx_entry.hpp", "uavx_ring_view.hpp"))
CSRC, LIB_PATH, HEADER = LIB.csrc, LIB.path, LIB.units[0].header
load, loaded, build, source_hash, _sources, _up_to_date, check = (LIB.load, LIB.loaded, LIB.build, LIB.source_hash,
                                                                  LIB.sources, LIB.up_to_date, LIB.check)

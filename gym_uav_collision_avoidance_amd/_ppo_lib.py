"""libuavx_ppo.so: PPO's sampling and loss heads (include/uavx_ppo.h), declared once: the constants of its
header, its one unit -- header, bound ABI version, every exported function with its restype and argtypes -- and
LIB = _native.Library(...) over it, which is sources, hash, build, staleness, load and bind.  The module's other names are
aliases of that object and of the table.  Its directory is its own; the clip, gae, ppo and norm libraries share the headers of
common_csrc/, whose code enters the source hash of each of the four; of those headers the actor, prio and keywalk libraries use
uavx_entry.hpp alone, and the env library none.  Nothing imports this module until a PPOHeads launches, and importing it neither builds nor maps anything.  There is NO
fallback: a missing library or device raises."""
import ctypes

from . import _native
from ._actor_lib import ERR_HIP, ERR_INVALID_ARG, OK  # noqa: F401  (the status codes are uavx_actor.h's)

BLOCK = 256                     # UAVX_PPO_BLOCK
PARTIAL_BYTES = 32              # workspace per workgroup: four float64

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
ABI_VERSION = 1

LIB = _native.Library("ppo_csrc", "libuavx_ppo.so", b"UAVX_PPO_SRC_HASH",
                      [_native.unit("ppo", "uavx_ppo.h", ABI_VERSION, FUNCTIONS)], extras=("uavx_actor.h",),
                      shared=("uavx_block_reduce.hpp", "uavx_entry.hpp"))
CSRC, LIB_PATH, HEADER = LIB.csrc, LIB.path, LIB.units[0].header
load, loaded, build, source_hash, _sources, _up_to_date, check = (LIB.load, LIB.loaded, LIB.build, LIB.source_hash,
                                                                  LIB.sources, LIB.up_to_date, LIB.check)

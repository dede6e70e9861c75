"""libuavx_keywalk.so: the n-step walk from the keys of a prioritized sample (include/uavx_keywalk.h),
declared once: the constants and the structure of its header, its one unit -- header, bound ABI version, every exported
function with its restype and argtypes -- and LIB = _native.Library(...) over it, which is sources, hash, build, staleness,
load and bind.  The module's other names are aliases of that object and of the table.  Its directory is its own; the n-step
walk itself, the replay ring's view and the entry-point plumbing are common_csrc/'s, shared with the actor library's replay
unit and the prio library, and their code enters its source hash.  There is NO fallback: a missing library or
device raises."""
import ctypes

from . import _native
from ._actor_lib import ERR_INVALID_ARG, OK, ReplayRing  # noqa: F401  (the ring and the status codes are uavx_replay.h's)

MAX_STEP = 8                    # UAVX_KEYWALK_MAX_STEP
MAX_ROWS = 1048576              # UAVX_KEYWALK_MAX_ROWS


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
ABI_VERSION = 1

LIB = _native.Library("keywalk_csrc", "libuavx_keywalk.so", b"UAVX_KEYWALK_SRC_HASH",
                      [_native.unit("key-walk", "uavx_keywalk.h", ABI_VERSION, FUNCTIONS)],
                      extras=("uavx_replay.h", "uavx_actor.h"),
                      shared=("uavx_entry.hpp", "uavx_replay_ring.hpp", "uavx_replay_walk.hpp"))
CSRC, LIB_PATH, HEADER = LIB.csrc, LIB.path, LIB.units[0].header
load, loaded, build, source_hash, _sources, _up_to_date, check = (LIB.load, LIB.loaded, LIB.build, LIB.source_hash,
                                                                  LIB.sources, LIB.up_to_date, LIB.check)

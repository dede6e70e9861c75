"""libuavx_prio.so: the prioritized-replay kernels (include/uavx_prio.h), declared once: the constants and
structures of its header, its one unit -- header, bound ABI version, every exported function with its restype and argtypes
-- and LIB = _native.Library(...) over it, which is sources, hash, build, staleness, load and bind.  The module's other names
are aliases of that object and of the table.  Its directory is its own; the replay ring's view and
the entry-point plumbing are common_csrc/'s, shared with the actor library's replay unit and the keywalk library, and their
code enters its source hash.  There is NO fallback: a missing library or device raises."""
import ctypes

from . import _native
from ._actor_lib import ERR_INVALID_ARG, OK, ReplayRing  # noqa: F401  (the ring and the status codes are uavx_replay.h's)

ONE = 65536                     # UAVX_PRIO_ONE: Q16.16
MAX_ENTRIES = 67108864          # UAVX_PRIO_MAX_ENTRIES
MAX_ROWS = 1048576              # UAVX_PRIO_MAX_ROWS
MAX_TOWERS = 2                  # UAVX_PRIO_MAX_TOWERS
FAN = 64                        # children per node of the partial sums
RECORD_BYTES = 32               # sizeof(uavx_prio_record)


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
ABI_VERSION = 1

LIB = _native.Library("prio_csrc", "libuavx_prio.so", b"UAVX_PRIO_SRC_HASH",
                      [_native.unit("prioritized-replay", "uavx_prio.h", ABI_VERSION, FUNCTIONS)],
                      extras=("uavx_replay.h", "uavx_actor.h"), shared=("uavx_entry.hpp", "uavx_replay_ring.hpp"))
CSRC, LIB_PATH, HEADER = LIB.csrc, LIB.path, LIB.units[0].header
load, loaded, build, source_hash, _sources, _up_to_date, check = (LIB.load, LIB.loaded, LIB.build, LIB.source_hash,
                                                                  LIB.sources, LIB.up_to_date, LIB.check)

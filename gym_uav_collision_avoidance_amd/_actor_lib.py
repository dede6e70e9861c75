"""ctypes binding of libuavx_actor.so (include/uavx_actor.h, include/uavx_critic.h, include/uavx_critic_grad.h,
include/uavx_optim.h, include/uavx_replay.h, include/uavx_action_grad.h, include/uavx_policy_grad.h,
include/uavx_learner.h, include/uavx_explore.h), the fused actor-inference, critic, TD-target, critic-gradient, optimiser-step, replay-sampling,
critic action-gradient, actor forward / backward, learner-tail and exploration kernels.  Built, checked for staleness and loaded like libuavx.so (_lib.py), from a directory of its own so
that the environment library and the source hash its profiles carry do not change with it.  There is NO fallback: a
missing library or device raises."""
import ctypes
import os

from . import _native

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "actor_csrc")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "uavx_actor.h")
CRITIC_HEADER = os.path.join(os.path.dirname(_HERE), "include", "uavx_critic.h")
GRAD_HEADER = os.path.join(os.path.dirname(_HERE), "include", "uavx_critic_grad.h")
OPTIM_HEADER = os.path.join(os.path.dirname(_HERE), "include", "uavx_optim.h")
REPLAY_HEADER = os.path.join(os.path.dirname(_HERE), "include", "uavx_replay.h")
ACTION_GRAD_HEADER = os.path.join(os.path.dirname(_HERE), "include", "uavx_action_grad.h")
POLICY_GRAD_HEADER = os.path.join(os.path.dirname(_HERE), "include", "uavx_policy_grad.h")
LEARNER_HEADER = os.path.join(os.path.dirname(_HERE), "include", "uavx_learner.h")
EXPLORE_HEADER = os.path.join(os.path.dirname(_HERE), "include", "uavx_explore.h")
LIB_PATH = os.path.join(CSRC, "libuavx_actor.so")
ABI_VERSION = 1

SAC, TD3, DDPG = 0, 1, 2
F32, BF16 = 0, 1
RAW, DETERMINISTIC, SAC_SAMPLE, ADD_CLAMP = 0, 1, 2, 3
OK, ERR_INVALID_ARG, ERR_HIP, ERR_UNSUPPORTED, ERR_NOT_PACKED = 0, -1, -2, -3, -4

# every symbol include/uavx_actor.h declares (tests check the built library exports each of them)
SYMBOLS = ("uavx_actor_version", "uavx_actor_strerror", "uavx_actor_create", "uavx_actor_destroy", "uavx_actor_pack",
           "uavx_actor_forward")
# every symbol include/uavx_critic.h declares
CRITIC_SYMBOLS = ("uavx_critic_version", "uavx_critic_strerror", "uavx_critic_create", "uavx_critic_destroy",
                  "uavx_critic_set_split_rows", "uavx_critic_pack", "uavx_critic_q", "uavx_critic_target")
CRITIC_ABI_VERSION = 1
SPLIT_ROWS = 16384      # UAVX_CRITIC_SPLIT_ROWS: batches below it run the small-batch variant
# every symbol include/uavx_critic_grad.h declares
GRAD_SYMBOLS = ("uavx_critic_grad_version", "uavx_critic_grad_workspace_bytes", "uavx_critic_grad")
GRAD_ABI_VERSION = 1
GRAD_MSE, GRAD_L1 = 0, 1
GRAD_MAX_ROWS = 262144  # UAVX_CRITIC_GRAD_MAX_ROWS
# every symbol include/uavx_optim.h declares
OPTIM_SYMBOLS = ("uavx_optim_version", "uavx_optim_adam", "uavx_optim_soft_update")
OPTIM_ABI_VERSION = 1
OPTIM_MAX_TENSORS = 16  # UAVX_OPTIM_MAX_TENSORS
# every symbol include/uavx_replay.h declares
REPLAY_SYMBOLS = ("uavx_replay_version", "uavx_replay_workspace_bytes", "uavx_replay_sample")
REPLAY_ABI_VERSION = 1
REPLAY_MAX_ROWS = 1048576   # UAVX_REPLAY_MAX_ROWS
REPLAY_SINGLE_ROWS = 1024   # UAVX_REPLAY_SINGLE_ROWS: up to here one launch and no workspace
# every symbol include/uavx_action_grad.h declares
ACTION_GRAD_SYMBOLS = ("uavx_action_grad_version", "uavx_action_grad")
ACTION_GRAD_ABI_VERSION = 1
ACTION_GRAD_MAX_ROWS = 262144   # UAVX_ACTION_GRAD_MAX_ROWS
# every symbol include/uavx_policy_grad.h declares
POLICY_GRAD_SYMBOLS = ("uavx_policy_grad_version", "uavx_policy_grad_workspace_bytes", "uavx_policy_grad_forward",
                       "uavx_policy_grad_backward")
POLICY_GRAD_ABI_VERSION = 1
POLICY_GRAD_MAX_ROWS = 262144   # UAVX_POLICY_GRAD_MAX_ROWS
# every symbol include/uavx_learner.h declares
LEARNER_SYMBOLS = ("uavx_learner_version", "uavx_learner_tail")
LEARNER_ABI_VERSION = 1
LEARNER_LOG_COLUMNS = 8         # UAVX_LEARNER_LOG_COLUMNS
# every symbol include/uavx_explore.h declares
EXPLORE_SYMBOLS = ("uavx_explore_version", "uavx_explore_act")
EXPLORE_ABI_VERSION = 1
EXPLORE_MAX_ROWS = 16777216     # UAVX_EXPLORE_MAX_ROWS
EXPLORE_STATE_BYTES = 16        # UAVX_EXPLORE_STATE_BYTES

_lib_handle = None


class ReplayRing(ctypes.Structure):
    """uavx_replay_ring of include/uavx_replay.h."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ("obs", "act", "rew", "done", "skip", "trunc", "ended")]
                + [(n, ctypes.c_int64) for n in ("slots", "envs", "agents", "learners")])


class ExploreArgs(ctypes.Structure):
    """uavx_explore_args of include/uavx_explore.h."""
    _fields_ = [("kind", ctypes.c_int32), ("rows_per_env", ctypes.c_int32), ("rows", ctypes.c_int64),
                ("row_offset", ctypes.c_int64), ("seed", ctypes.c_uint64), ("raw", ctypes.c_void_p),
                ("raw_stride", ctypes.c_int64), ("out", ctypes.c_void_p), ("out_stride", ctypes.c_int64),
                ("state", ctypes.c_void_p), ("normals", ctypes.c_void_p), ("normals_out", ctypes.c_void_p),
                ("reset_flags", ctypes.c_void_p), ("reset_stride", ctypes.c_int64), ("reset_mask", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("warmup_steps", ctypes.c_int64), ("random_prob_dev", ctypes.c_void_p),
                ("random_prob", ctypes.c_float), ("noise_std", ctypes.c_float), ("ou_sigma", ctypes.c_double),
                ("ou_theta", ctypes.c_double), ("ou_dt", ctypes.c_double), ("ou_mean", ctypes.c_double),
                ("ou_x_initial", ctypes.c_double)]


def _sources():
    import glob
    return (sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
            + [HEADER, CRITIC_HEADER, GRAD_HEADER, OPTIM_HEADER, REPLAY_HEADER, ACTION_GRAD_HEADER,
               POLICY_GRAD_HEADER, LEARNER_HEADER, EXPLORE_HEADER])


def source_hash():
    """sha256 over the code (comments and whitespace dropped) of actor_csrc/*.hip, *.hpp and the nine headers of include/, plus
    the Makefile without comments and any HIPCC / ARCH / HIPFLAGS override (_native.source_hash); 16 hex digits."""
    return _native.source_hash(CSRC, _sources())


def build(force=False):
    """hipcc build of actor_csrc/ into libuavx_actor.so (gfx950), under a file lock and renamed into place (_native.build)."""
    return _native.build(CSRC, LIB_PATH, source_hash, _up_to_date, force)


def _up_to_date():
    """Does LIB_PATH carry the hash of the sources in the tree (read from the file, not through dlopen)?"""
    return _native.up_to_date(CSRC, LIB_PATH, b"UAVX_ACTOR_SRC_HASH", _sources(), source_hash)


def load():
    global _lib_handle
    if _lib_handle is not None:
        return _lib_handle
    if not os.path.exists(LIB_PATH) or not _up_to_date():
        build()                 # a build, not a fallback: a compile error is raised as such
    L = ctypes.CDLL(LIB_PATH)
    vp, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    L.uavx_actor_version.restype = i32
    if L.uavx_actor_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks actor ABI version {L.uavx_actor_version()}, this package binds {ABI_VERSION}: "
                           f"rebuild it (`make -B -C {CSRC}`)")
    L.uavx_actor_strerror.restype = ctypes.c_char_p
    L.uavx_actor_strerror.argtypes = [i32]
    L.uavx_actor_create.argtypes = [i32, i32, i32, i32, i32, i32, ctypes.POINTER(vp)]
    L.uavx_actor_destroy.argtypes = [vp]
    L.uavx_actor_pack.argtypes = [vp] + [vp] * 8 + [vp]
    L.uavx_actor_forward.argtypes = [vp, vp, i64, i64, vp, f32, i32, vp, i64, vp]
    L.uavx_critic_version.restype = i32
    if L.uavx_critic_version() != CRITIC_ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks critic ABI version {L.uavx_critic_version()}, this package binds "
                           f"{CRITIC_ABI_VERSION}: rebuild it (`make -B -C {CSRC}`)")
    L.uavx_critic_strerror.restype = ctypes.c_char_p
    L.uavx_critic_strerror.argtypes = [i32]
    L.uavx_critic_create.argtypes = [i32, i32, i32, i32, i32, i32, ctypes.POINTER(vp)]
    L.uavx_critic_destroy.argtypes = [vp]
    L.uavx_critic_set_split_rows.argtypes = [vp, i64]
    L.uavx_critic_pack.argtypes = [vp] + [vp] * 12 + [vp]
    L.uavx_critic_q.argtypes = [vp, vp, i64, i64, vp, i64, vp, i64, vp]
    L.uavx_critic_target.argtypes = [vp, vp, vp, i64, i64, vp, i64, vp, i64, vp, vp, f32, f32, f32, vp, i64, vp, i64, vp]
    L.uavx_critic_grad_version.restype = i32
    if L.uavx_critic_grad_version() != GRAD_ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks critic-gradient ABI version {L.uavx_critic_grad_version()}, this package "
                           f"binds {GRAD_ABI_VERSION}: rebuild it (`make -B -C {CSRC}`)")
    L.uavx_critic_grad_workspace_bytes.argtypes = [vp, i64, ctypes.POINTER(i64)]
    L.uavx_critic_grad.argtypes = [vp, i32, ctypes.POINTER(vp), vp, i64, i64, vp, i64, vp, i64, ctypes.POINTER(vp), vp, vp,
                                   i64, vp]
    L.uavx_optim_version.restype = i32
    if L.uavx_optim_version() != OPTIM_ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks optimiser ABI version {L.uavx_optim_version()}, this package binds "
                           f"{OPTIM_ABI_VERSION}: rebuild it (`make -B -C {CSRC}`)")
    f64, pvp, pi64 = ctypes.c_double, ctypes.POINTER(vp), ctypes.POINTER(i64)
    L.uavx_optim_adam.argtypes = [i32, pvp, pvp, pvp, pvp, pvp, pvp, pi64, f64, f64, f64, f64, f64, vp, vp, vp]
    L.uavx_optim_soft_update.argtypes = [i32, pvp, pvp, pi64, f64, vp]
    L.uavx_replay_version.restype = i32
    if L.uavx_replay_version() != REPLAY_ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks replay ABI version {L.uavx_replay_version()}, this package binds "
                           f"{REPLAY_ABI_VERSION}: rebuild it (`make -B -C {CSRC}`)")
    L.uavx_replay_workspace_bytes.argtypes = [i64, pi64]
    L.uavx_replay_sample.argtypes = [ctypes.POINTER(ReplayRing), i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]
    L.uavx_action_grad_version.restype = i32
    if L.uavx_action_grad_version() != ACTION_GRAD_ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks action-gradient ABI version {L.uavx_action_grad_version()}, this package "
                           f"binds {ACTION_GRAD_ABI_VERSION}: rebuild it (`make -B -C {CSRC}`)")
    L.uavx_action_grad.argtypes = [vp, i32, pvp, vp, i64, i64, vp, i64, vp, vp, vp]
    L.uavx_policy_grad_version.restype = i32
    if L.uavx_policy_grad_version() != POLICY_GRAD_ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks policy-gradient ABI version {L.uavx_policy_grad_version()}, this package "
                           f"binds {POLICY_GRAD_ABI_VERSION}: rebuild it (`make -B -C {CSRC}`)")
    L.uavx_policy_grad_workspace_bytes.argtypes = [i32, i32, i32, i64, pi64]
    L.uavx_policy_grad_forward.argtypes = [i32, i32, i32, pvp, vp, i64, i64, vp, vp, vp, vp, i64, vp]
    L.uavx_policy_grad_backward.argtypes = [i32, i32, i32, pvp, vp, i64, i64, vp, vp, i64, f32, vp, pvp, vp, vp, vp, i64, vp]
    L.uavx_learner_version.restype = i32
    if L.uavx_learner_version() != LEARNER_ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks learner ABI version {L.uavx_learner_version()}, this package binds "
                           f"{LEARNER_ABI_VERSION}: rebuild it (`make -B -C {CSRC}`)")
    L.uavx_learner_tail.argtypes = [i32, pvp, vp, f32, vp, vp, vp, vp, f64, f64, f64, f64, vp, vp, i64, vp, i32, vp]
    L.uavx_explore_version.restype = i32
    if L.uavx_explore_version() != EXPLORE_ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks exploration ABI version {L.uavx_explore_version()}, this package binds "
                           f"{EXPLORE_ABI_VERSION}: rebuild it (`make -B -C {CSRC}`)")
    L.uavx_explore_act.argtypes = [ctypes.POINTER(ExploreArgs), vp]
    _lib_handle = L
    return L


def check(rc, what):
    if rc != OK:
        raise RuntimeError(f"uavx: {what} failed: {load().uavx_actor_strerror(rc).decode()} ({rc})")


def check_critic(rc, what):
    if rc != OK:
        raise RuntimeError(f"uavx: {what} failed: {load().uavx_critic_strerror(rc).decode()} ({rc})")

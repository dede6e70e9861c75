"""libuavx_actor.so: the fused actor, critic, TD-target, gradient, optimiser, replay, learner-tail and exploration kernels,
declared once.  UNITS describes its eleven units -- header, bound ABI version, every exported function with its restype and
argtypes -- and LIB = _native.Library(...) over them is everything else: sources, hash, build, staleness, load and bind.  The
module's other names are aliases of that object and of the table.  Its directory is its own, so that the environment library
and the source hash its profiles carry do not change with it; its replay unit shares the replay ring's view and the n-step
walk of common_csrc/ with the prio and keywalk libraries, and their code enters its source hash.  There is NO fallback: a missing library or device raises."""
import ctypes

from . import _native
from ._native import Unit, unit as _unit  # noqa: F401

SAC, TD3, DDPG = 0, 1, 2
F32, BF16 = 0, 1
RAW, DETERMINISTIC, SAC_SAMPLE, ADD_CLAMP = 0, 1, 2, 3
OK, ERR_INVALID_ARG, ERR_HIP, ERR_UNSUPPORTED, ERR_NOT_PACKED = 0, -1, -2, -3, -4

SPLIT_ROWS = 16384              # UAVX_CRITIC_SPLIT_ROWS: batches below it run the small-batch variant
GRAD_MSE, GRAD_L1 = 0, 1
GRAD_MAX_ROWS = 262144          # UAVX_CRITIC_GRAD_MAX_ROWS
OPTIM_MAX_TENSORS = 16          # UAVX_OPTIM_MAX_TENSORS
REPLAY_MAX_ROWS = 1048576       # UAVX_REPLAY_MAX_ROWS
REPLAY_SINGLE_ROWS = 1024       # UAVX_REPLAY_SINGLE_ROWS: up to here one launch and no workspace
ACTION_GRAD_MAX_ROWS = 262144   # UAVX_ACTION_GRAD_MAX_ROWS
POLICY_GRAD_MAX_ROWS = 262144   # UAVX_POLICY_GRAD_MAX_ROWS
LEARNER_LOG_COLUMNS = 8         # UAVX_LEARNER_LOG_COLUMNS
EXPLORE_MAX_ROWS = 16777216     # UAVX_EXPLORE_MAX_ROWS
EXPLORE_STATE_BYTES = 16        # UAVX_EXPLORE_STATE_BYTES
NSTEP_MAX = 8                   # UAVX_NSTEP_MAX
NSTEP_MAX_ROWS = 1048576        # UAVX_NSTEP_MAX_ROWS
NSTEP_SINGLE_ROWS = 1024        # UAVX_NSTEP_SINGLE_ROWS: up to here one launch and no workspace


class ReplayRing(ctypes.Structure):
    """uavx_replay_ring of include/uavx_replay.h."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ("obs", "act", "rew", "done", "skip", "trunc", "ended")]
                + [(n, ctypes.c_int64) for n in ("slots", "envs", "agents", "learners")])


class NStepArgs(ctypes.Structure):
    """uavx_nstep_args of include/uavx_nstep.h."""
    _fields_ = [("ring", ctypes.POINTER(ReplayRing)), ("count", ctypes.c_int64), ("count_dev", ctypes.c_void_p),
                ("u", ctypes.c_void_p), ("u_cols", ctypes.c_int32), ("n_step", ctypes.c_int32), ("gamma", ctypes.c_double),
                ("recency", ctypes.c_float), ("rows", ctypes.c_int64), ("state", ctypes.c_void_p),
                ("action", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("next_state", ctypes.c_void_p),
                ("mask", ctypes.c_void_p), ("length", ctypes.c_void_p), ("truncated", ctypes.c_void_p),
                ("ended", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64)]


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


_vp, _i64, _i32, _f32, _f64, _str = (ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_double,
                                 ctypes.c_char_p)
_pvp, _pi64 = ctypes.POINTER(_vp), ctypes.POINTER(_i64)

UNITS = (
    _unit("actor", "uavx_actor.h", 1, {
        "uavx_actor_version": (_i32, []),
        "uavx_actor_strerror": (_str, [_i32]),
        "uavx_actor_create": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _pvp]),
        "uavx_actor_destroy": (_i32, [_vp]),
        "uavx_actor_pack": (_i32, [_vp] + [_vp] * 8 + [_vp]),
        "uavx_actor_forward": (_i32, [_vp, _vp, _i64, _i64, _vp, _f32, _i32, _vp, _i64, _vp])}),
    _unit("critic", "uavx_critic.h", 1, {
        "uavx_critic_version": (_i32, []),
        "uavx_critic_strerror": (_str, [_i32]),
        "uavx_critic_create": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _pvp]),
        "uavx_critic_destroy": (_i32, [_vp]),
        "uavx_critic_set_split_rows": (_i32, [_vp, _i64]),
        "uavx_critic_pack": (_i32, [_vp] + [_vp] * 12 + [_vp]),
        "uavx_critic_q": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp]),
        "uavx_critic_target": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _f32, _f32, _f32, _vp,
                                      _i64, _vp, _i64, _vp])}),
    _unit("critic-gradient", "uavx_critic_grad.h", 1, {
        "uavx_critic_grad_version": (_i32, []),
        "uavx_critic_grad_workspace_bytes": (_i32, [_vp, _i64, _pi64]),
        "uavx_critic_grad": (_i32, [_vp, _i32, _pvp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _pvp, _vp, _vp, _i64, _vp])}),
    _unit("optimiser", "uavx_optim.h", 1, {
        "uavx_optim_version": (_i32, []),
        "uavx_optim_adam": (_i32, [_i32, _pvp, _pvp, _pvp, _pvp, _pvp, _pvp, _pi64, _f64, _f64, _f64, _f64, _f64, _vp,
                                   _vp, _vp]),
        "uavx_optim_soft_update": (_i32, [_i32, _pvp, _pvp, _pi64, _f64, _vp])}),
    _unit("replay", "uavx_replay.h", 1, {
        "uavx_replay_version": (_i32, []),
        "uavx_replay_workspace_bytes": (_i32, [_i64, _pi64]),
        "uavx_replay_sample": (_i32, [ctypes.POINTER(ReplayRing), _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _i64, _vp])}),
    _unit("action-gradient", "uavx_action_grad.h", 1, {
        "uavx_action_grad_version": (_i32, []),
        "uavx_action_grad": (_i32, [_vp, _i32, _pvp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp])}),
    _unit("policy-gradient", "uavx_policy_grad.h", 1, {
        "uavx_policy_grad_version": (_i32, []),
        "uavx_policy_grad_workspace_bytes": (_i32, [_i32, _i32, _i32, _i64, _pi64]),
        "uavx_policy_grad_forward": (_i32, [_i32, _i32, _i32, _pvp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
        "uavx_policy_grad_backward": (_i32, [_i32, _i32, _i32, _pvp, _vp, _i64, _i64, _vp, _vp, _i64, _f32, _vp, _pvp,
                                             _vp, _vp, _vp, _i64, _vp])}),
    _unit("learner", "uavx_learner.h", 1, {
        "uavx_learner_version": (_i32, []),
        "uavx_learner_tail": (_i32, [_i32, _pvp, _vp, _f32, _vp, _vp, _vp, _vp, _f64, _f64, _f64, _f64, _vp, _vp, _i64,
                                     _vp, _i32, _vp])}),
    _unit("exploration", "uavx_explore.h", 1, {
        "uavx_explore_version": (_i32, []),
        "uavx_explore_act": (_i32, [ctypes.POINTER(ExploreArgs), _vp])}),
    _unit("n-step replay", "uavx_nstep.h", 1, {
        "uavx_nstep_version": (_i32, []),
        "uavx_nstep_workspace_bytes": (_i32, [_i64, _pi64]),
        "uavx_nstep_sample": (_i32, [ctypes.POINTER(NStepArgs), _vp])}),
    _unit("weighted critic-gradient", "uavx_wcritic_grad.h", 1, {
        "uavx_wcritic_grad_version": (_i32, []),
        "uavx_wcritic_grad_workspace_bytes": (_i32, [_i32, _i32, _i32, _i32, _i64, _pi64]),
        "uavx_wcritic_grad": (_i32, [_i32, _i32, _i32, _i32, _i32, _pvp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64,
                                     _pvp, _vp, _vp, _vp, _i64, _vp])}),
)
(HEADER, CRITIC_HEADER, GRAD_HEADER, OPTIM_HEADER, REPLAY_HEADER, ACTION_GRAD_HEADER, POLICY_GRAD_HEADER, LEARNER_HEADER,
 EXPLORE_HEADER, NSTEP_HEADER, WGRAD_HEADER) = (u.header for u in UNITS)
(SYMBOLS, CRITIC_SYMBOLS, GRAD_SYMBOLS, OPTIM_SYMBOLS, REPLAY_SYMBOLS, ACTION_GRAD_SYMBOLS, POLICY_GRAD_SYMBOLS,
 LEARNER_SYMBOLS, EXPLORE_SYMBOLS, NSTEP_SYMBOLS, WGRAD_SYMBOLS) = (tuple(u.functions) for u in UNITS)
(ABI_VERSION, CRITIC_ABI_VERSION, GRAD_ABI_VERSION, OPTIM_ABI_VERSION, REPLAY_ABI_VERSION, ACTION_GRAD_ABI_VERSION,
 POLICY_GRAD_ABI_VERSION, LEARNER_ABI_VERSION, EXPLORE_ABI_VERSION, NSTEP_ABI_VERSION,
 WGRAD_ABI_VERSION) = (u.abi for u in UNITS)

LIB = _native.Library("actor_csrc", "libuavx_actor.so", b"UAVX_ACTOR_SRC_HASH", UNITS,
                      shared=("uavx_entry.hpp", "uavx_replay_ring.hpp", "uavx_replay_walk.hpp"))
CSRC, LIB_PATH = LIB.csrc, LIB.path
load, loaded, build, source_hash, _sources, _up_to_date = (LIB.load, LIB.loaded, LIB.build, LIB.source_hash, LIB.sources,
                                                           LIB.up_to_date)


def check(rc, what):
    if rc != OK:
        raise RuntimeError(f"uavx: {what} failed: {load().uavx_actor_strerror(rc).decode()} ({rc})")


def check_critic(rc, what):
    if rc != OK:
        raise RuntimeError(f"uavx: {what} failed: {load().uavx_critic_strerror(rc).decode()} ({rc})")


# uavx_wcritic_grad.h has no strerror of its own, and uavx_critic_strerror words two of its three codes otherwise
check_wgrad = LIB.check

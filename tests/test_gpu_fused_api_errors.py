"""Every per-call rejection of the fused learner bindings (fused_critic.py, fused_policy_grad.py, fused_replay.py,
learners.py, and the checks of _fused_common.py behind them) pinned, exception class and message, to what the parent of
the change that gave them one home raised: tests/golden/fused_api_errors_parent.json, recorded there once by
tests/golden/make_fused_api_errors.py from CASES below.  Default-size modules on cuda:0; valid arguments have 1, 3 or 17
rows (17 crosses the 16-row tile, 1 takes the stride-defaulting branch of the row checks); the MAX_ROWS + 1 cases pass
expanded views of one row, so nothing large is allocated; the capture cases enter torch.cuda.graph with an unreserved
object and the call under test enqueues nothing."""
import functools
import json
import os

import pytest
import torch

from gym_uav_collision_avoidance_amd import _actor_lib, policy

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_api_errors_parent.json")
KINDS = ("sac", "td3", "ddpg")
ACTORS = {"sac": policy.GaussianPolicy, "td3": policy.TD3Actor, "ddpg": policy.DDPGActor}
CRITICS = {"sac": policy.TwinQ, "td3": policy.TD3TwinQ, "ddpg": policy.DDPGCritic}
ROWS = {"sac": 17, "td3": 3, "ddpg": 1}
CASES = {}      # id -> a function of no arguments that must raise


def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def obj(what, kind):
    """One object of each class per learner kind, built on first use and shared by the cases (they only get refused)."""
    from gym_uav_collision_avoidance_amd import fused_critic as fc, learners
    from gym_uav_collision_avoidance_amd.fused_actor import FusedActor
    from gym_uav_collision_avoidance_amd.fused_policy_grad import FusedPolicyGrad
    if what == "actor":
        return ACTORS[kind]().to(dev())
    if what == "critic":
        return CRITICS[kind]().to(dev())
    if what == "fused_critic":
        return fc.FusedCritic(obj("critic", kind))
    if what == "target":
        return fc.FusedTarget(FusedActor(obj("actor", kind)), obj("fused_critic", kind))
    if what == "closs":
        return fc.FusedCriticLoss(obj("fused_critic", kind))
    if what == "qa":
        return fc.FusedActionGrad(obj("fused_critic", kind))
    if what == "aloss":
        return fc.FusedActorLoss(obj("actor", kind), obj("qa", kind))
    if what == "pg":
        return FusedPolicyGrad(obj("actor", kind), obj("qa", kind))
    if what == "agent":
        return {"sac": learners.FusedSAC, "td3": learners.FusedTD3, "ddpg": learners.FusedDDPG}[kind](device=dev())
    raise KeyError(what)


def z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device=dev())


def good(kind):
    """Valid (state, action, reward, next_state, mask) of the kind's row count."""
    b = ROWS[kind]
    return z(b, 10), z(b, 2), z(b), z(b, 10), z(b, 1)


def bad_matrix(rows, cols, optional=False):
    """name -> a stand-in for a float32 [rows, cols] device tensor that the row checks refuse (None, unless it means
    "not given")."""
    bad = {"dtype": lambda: z(rows, cols, dtype=torch.float64), "cpu": lambda: torch.zeros(rows, cols),
           "rank": lambda: z(rows * cols), "cols": lambda: z(rows, cols + 1),
           "last_stride": lambda: z(rows, 2 * cols)[:, ::2]}
    return bad if optional else dict(bad, none=lambda: None)


def bad_column(rows):
    return {"dtype": lambda: z(rows, dtype=torch.float64), "cpu": lambda: torch.zeros(rows),
            "shape": lambda: z(rows, 2), "rows": lambda: z(rows + 1)}


def bad_buffer(*shape):
    """name -> a stand-in for a contiguous float32 device tensor of `shape`."""
    wide = shape[:-1] + (2 * shape[-1],)
    bad = {"dtype": lambda: z(*shape, dtype=torch.float64), "cpu": lambda: torch.zeros(shape),
           "shape": lambda: z(*shape[:-1], shape[-1] + 1)}
    return dict(bad, strided=lambda: z(*wide)[..., ::2]) if shape[-1] > 1 else bad      # one column is always contiguous


def case(name):
    def register(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return register


def add(name, call, **fixed):
    """Registers call(**fixed, **{arg: bad()}) for every (arg, {variant: bad}) given through add(...)(arg=variants)."""
    def with_bad(**bads):
        for arg, variants in bads.items():
            for variant, make in variants.items():
                assert f"{name}-{arg}-{variant}" not in CASES, (name, arg, variant)
                CASES[f"{name}-{arg}-{variant}"] = (lambda arg=arg, make=make: call(**{**fixed, arg: make()}))
    return with_bad


def in_capture(call):
    """Runs `call` inside a graph capture that already holds one launch of its own; the exception leaves the capture."""
    scratch = z(8)
    torch.cuda.synchronize()
    try:
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            scratch.add_(1)
            call()
    finally:
        torch.cuda.synchronize()


def big(cols=None):
    """MAX_ROWS + 1 rows (the three gradient units share the limit) as an expanded view of one row."""
    n = _actor_lib.GRAD_MAX_ROWS + 1
    return z(1).expand(n) if cols is None else z(1, cols).expand(n, cols)


def unusable(param):
    """Makes a parameter non-contiguous in place (same values, same shape)."""
    param.data = param.data.t().contiguous().t()


# ---- FusedCritic.q ------------------------------------------------------------------------------------------------------
def _q(kind="td3", **kw):
    s, a = good(kind)[:2]
    return obj("fused_critic", kind).q(**{**dict(state=s, action=a), **kw})


for _k in KINDS:
    add(f"{_k}-critic.q", _q, kind=_k)(state=bad_matrix(ROWS[_k], 10), action=bad_matrix(ROWS[_k], 2))
add("critic.q", _q)(action={"rows": lambda: z(4, 2)}, out=dict(bad_matrix(3, 2, optional=True), rows=lambda: z(4, 2)))
add("ddpg-critic.q", _q, kind="ddpg")(out={"cols": lambda: z(1, 2)})


# ---- FusedTarget ----------------------------------------------------------------------------------------------------------
def _target(kind, **kw):
    _, _, r, s2, m = good(kind)
    args = dict(next_state=s2, reward=r, mask=m)
    if kind == "sac":
        args["alpha"] = 0.2
    args.update(kw)
    return obj("target", kind)(**args)


for _k in KINDS:
    _b = ROWS[_k]
    add(f"{_k}-target", _target, kind=_k)(next_state=bad_matrix(_b, 10), reward=bad_column(_b), mask=bad_column(_b),
                                          out=bad_column(_b),
                                          aux=dict(bad_matrix(_b, 4, optional=True), rows=lambda b=_b: z(b + 1, 4)))
for _k in ("sac", "td3"):
    _b = ROWS[_k]
    add(f"{_k}-target", _target, kind=_k)(noise=dict(bad_matrix(_b, 2, optional=True), rows=lambda b=_b: z(b + 1, 2),
                                                     row_stride=lambda b=_b: z(b, 4)[:, :2]))
add("sac-target", _target, kind="sac")(alpha={"missing": lambda: None, "two": lambda: z(2), "cpu": lambda: torch.zeros(1),
                                              "dtype": lambda: z(1, dtype=torch.float64)})


# ---- FusedCriticLoss ------------------------------------------------------------------------------------------------------
def _closs(kind, **kw):
    s, a, r = good(kind)[:3]
    return obj("closs", kind).backward(**{**dict(state=s, action=a, y=r), **kw})


for _k in KINDS:
    _b = ROWS[_k]
    add(f"{_k}-closs", _closs, kind=_k)(state=bad_matrix(_b, 10), y=bad_column(_b),
                                        action=dict(bad_matrix(_b, 2), rows=lambda b=_b: z(b + 1, 2)))
case("closs-rows-0")(lambda: _closs("td3", state=z(0, 10), action=z(0, 2), y=z(0)))
case("closs-rows-max+1")(lambda: _closs("td3", state=big(10), action=big(2), y=big()))


def _fresh_closs(kind="td3"):
    from gym_uav_collision_avoidance_amd.fused_critic import FusedCriticLoss
    return FusedCriticLoss(CRITICS[kind]().to(dev()))


@case("closs-parameter-not-contiguous")
def _():
    cl = _fresh_closs()
    try:
        unusable(cl.module.l2.weight)
        cl.backward(*good("td3")[:3])
    finally:
        cl.close()


@case("closs-capture-unreserved")
def _():
    cl = _fresh_closs("sac")
    try:
        s, a, y = good("sac")[:3]
        in_capture(lambda: cl.backward(s, a, y))
    finally:
        cl.close()


# ---- FusedActionGrad ------------------------------------------------------------------------------------------------------
def _qa(kind, **kw):
    s, a = good(kind)[:2]
    return obj("qa", kind).q_dqda(**{**dict(state=s, action=a), **kw})


for _k in KINDS:
    _b, _t = ROWS[_k], (1 if _k == "ddpg" else 2)
    add(f"{_k}-qa", _qa, kind=_k)(state=bad_matrix(_b, 10), action=dict(bad_matrix(_b, 2), rows=lambda b=_b: z(b + 1, 2)),
                                  towers={"bool": lambda: True, "str": lambda: "1", "zero": lambda: 0, "beyond": lambda: 4})
    for _v, _make in bad_buffer(_t, _b).items():
        case(f"{_k}-qa-out0-{_v}")(lambda k=_k, t=_t, b=_b, make=_make: _qa(k, out=(make(), z(t, b, 2))))
    for _v, _make in bad_buffer(_t, _b, 2).items():
        case(f"{_k}-qa-out1-{_v}")(lambda k=_k, t=_t, b=_b, make=_make: _qa(k, out=(z(t, b), make())))
case("ddpg-qa-towers-second")(lambda: _qa("ddpg", towers=2))
case("qa-rows-0")(lambda: _qa("td3", state=z(0, 10), action=z(0, 2)))
case("qa-rows-max+1")(lambda: _qa("td3", state=big(10), action=big(2)))
case("qa-call-towers-beyond")(lambda: obj("qa", "td3")(*good("td3")[:2], towers=8))


@case("qa-parameter-not-contiguous")
def _():
    from gym_uav_collision_avoidance_amd.fused_critic import FusedActionGrad
    qa = FusedActionGrad(policy.DDPGCritic().to(dev()))
    try:
        unusable(qa.module.fc1.weight)
        qa.q_dqda(*good("ddpg")[:2])
    finally:
        qa.close()


# ---- FusedActorLoss -------------------------------------------------------------------------------------------------------
def _aloss(kind, **kw):
    args = dict(state=good(kind)[0])
    if kind == "sac":
        args["alpha"] = 0.2
    return obj("aloss", kind).backward(**{**args, **kw})


for _k in KINDS:
    add(f"{_k}-aloss", _aloss, kind=_k)(state=bad_matrix(ROWS[_k], 10))
case("aloss-rows-0")(lambda: _aloss("td3", state=z(0, 10)))
case("aloss-rows-max+1")(lambda: _aloss("td3", state=big(10)))
add("sac-aloss", _aloss, kind="sac")(
    alpha={"missing": lambda: None, "cpu": lambda: torch.zeros(1), "dtype": lambda: z(1, dtype=torch.float64)},
    noise={"dtype": lambda: z(17, 2, dtype=torch.float64), "cpu": lambda: torch.zeros(17, 2), "rows": lambda: z(16, 2),
           "cols": lambda: z(17, 3), "rank": lambda: z(34)})


# ---- FusedPolicyGrad ------------------------------------------------------------------------------------------------------
def _pg(kind, method="backward", **kw):
    args = dict(state=good(kind)[0])
    if kind == "sac" and method == "backward":
        args["alpha"] = 0.2
    return getattr(obj("pg", kind), method)(**{**args, **kw})


_SAC_NOISE = {"dtype": lambda: z(17, 2, dtype=torch.float64), "cpu": lambda: torch.zeros(17, 2), "rows": lambda: z(16, 2),
              "cols": lambda: z(17, 3), "strided": lambda: z(17, 4)[:, :2]}
_SAC_ALPHA = {"missing": lambda: None, "two": lambda: z(2), "cpu": lambda: torch.zeros(1),
              "dtype": lambda: z(1, dtype=torch.float64)}
for _k in KINDS:
    add(f"{_k}-pg.backward", _pg, kind=_k)(state=bad_matrix(ROWS[_k], 10))
    add(f"{_k}-pg.act", _pg, kind=_k, method="act")(state=bad_matrix(ROWS[_k], 10))
for _m in ("backward", "act"):
    case(f"pg.{_m}-rows-0")(lambda m=_m: _pg("td3", m, state=z(0, 10)))
    case(f"pg.{_m}-rows-max+1")(lambda m=_m: _pg("td3", m, state=big(10)))
    add(f"sac-pg.{_m}", _pg, kind="sac", method=_m)(noise=_SAC_NOISE)
add("sac-pg.backward", _pg, kind="sac")(alpha=_SAC_ALPHA)
case("td3-pg-log_pi_mean")(lambda: obj("pg", "td3").log_pi_mean)


def _fresh_pg(kind):
    from gym_uav_collision_avoidance_amd.fused_policy_grad import FusedPolicyGrad
    return FusedPolicyGrad(ACTORS[kind]().to(dev()), obj("qa", kind))


def _backward_from(kind, act=True, **kw):
    """backward_from on a block of its own: after act() on the same rows unless act=False."""
    pg, (s, t, b) = _fresh_pg(kind), (good(kind)[0], 1 if kind == "ddpg" else 2, ROWS[kind])
    if act:
        pg.act(s)
    args = dict(state=s, q=z(t, b), dqda=z(t, b, 2))
    if kind == "sac":
        args["alpha"] = 0.2
    return pg.backward_from(**{**args, **kw})


for _k in KINDS:
    _b, _t = ROWS[_k], (1 if _k == "ddpg" else 2)
    add(f"{_k}-pg.backward_from", _backward_from, kind=_k, act=False)(
        state=bad_matrix(_b, 10), q=bad_buffer(_t, _b), dqda=bad_buffer(_t, _b, 2))
    case(f"{_k}-pg.backward_from-without-act")(lambda k=_k: _backward_from(k, act=False))
add("sac-pg.backward_from", _backward_from, kind="sac")(alpha=_SAC_ALPHA)


@case("pg.backward_from-other-rows")
def _():
    pg = _fresh_pg("td3")
    pg.act(z(17, 10))
    pg.backward_from(z(3, 10), z(2, 3), z(2, 3, 2))


@case("pg-parameter-not-contiguous")
def _():
    pg = _fresh_pg("td3")
    unusable(pg.actor.l2.weight)
    pg.act(good("td3")[0])


@case("pg.act-capture-unreserved")
def _():
    pg, s, eps = _fresh_pg("sac"), good("sac")[0], z(17, 2)
    in_capture(lambda: pg.act(s, noise=eps))


@case("pg.backward-capture-unreserved")
def _():
    pg, s = _fresh_pg("td3"), good("td3")[0]
    in_capture(lambda: pg.backward(s))


# ---- the learners' update_batch -------------------------------------------------------------------------------------------
def _update(kind, **kw):
    s, a, r, s2, m = good(kind)
    return obj("agent", kind).update_batch(**{**dict(s=s, a=a, r=r, s2=s2, mask=m), **kw})


for _k in KINDS:
    _b = ROWS[_k]
    _m10 = {k: v for k, v in bad_matrix(_b, 10).items() if k != "last_stride"}      # the blocks behind it check the strides
    _m2 = {k: v for k, v in bad_matrix(_b, 2).items() if k != "last_stride"}
    add(f"{_k}-update_batch", _update, kind=_k)(s=_m10, a=dict(_m2, rows=lambda b=_b: z(b + 1, 2)),
                                                s2=dict(_m10, rows=lambda b=_b: z(b + 1, 10)), r=bad_column(_b),
                                                mask=bad_column(_b))
    case(f"{_k}-update_batch-rows-0")(lambda k=_k: _update(k, s=z(0, 10), a=z(0, 2), s2=z(0, 10), r=z(0), mask=z(0)))
add("ddpg-update_batch", _update, kind="ddpg")(noise={"given": lambda: z(1, 2)})
add("sac-update_batch", _update, kind="sac")(noise={
    "one": lambda: z(17, 2), "three": lambda: (z(17, 2),) * 3, "dtype": lambda: (z(17, 2), z(17, 2, dtype=torch.float64)),
    "cpu": lambda: (torch.zeros(17, 2), z(17, 2)), "rows": lambda: (z(17, 2), z(16, 2)),
    "strided": lambda: (z(17, 4)[:, :2], z(17, 2)), "none": lambda: (None, z(17, 2))})
add("td3-update_batch", _update, kind="td3")(noise={"two": lambda: (z(3, 2), z(3, 2)), "cols": lambda: z(3, 3),
                                                     "strided": lambda: z(3, 4)[:, ::2]})


@case("update_batch-capture-unreserved")
def _():
    from gym_uav_collision_avoidance_amd.learners import FusedDDPG
    agent = FusedDDPG(device=dev())
    try:
        batch = good("ddpg")
        in_capture(lambda: agent.update_batch(*batch))
    finally:
        agent.close()


# ---- FusedReplaySampler ---------------------------------------------------------------------------------------------------
@case("replay.sample-capture-unreserved")
def _():
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.fused_replay import FusedReplaySampler
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    env = BatchedMultiUAVWorld2D(4, num_agents=2, device=dev(), seed=1)
    try:
        mem = DeviceReplay(env, horizon=4)
        mem.begin(env.reset())
        mem.action_slot().zero_()
        mem.step(polar=True)
        rows = _actor_lib.REPLAY_SINGLE_ROWS + 1            # the smallest batch that needs a workspace
        sampler, u = FusedReplaySampler(mem), z(2, 3, rows)
        in_capture(lambda: sampler.sample_from_uniforms(u))
    finally:
        torch.cuda.synchronize()
        env.close()


def outcome(fn):
    """[exception class name, message] of a case, or ["", ...] if it raised nothing."""
    try:
        fn()
    except Exception as e:      # noqa: BLE001 -- whatever it is, it is compared with the record
        return [type(e).__name__, str(e)]
    return ["", "raised nothing"]


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
def test_the_record_holds_exactly_the_cases_run_here(recorded):
    assert sorted(recorded) == sorted(CASES)
    assert all(cls for cls, _ in recorded.values()), [k for k, v in recorded.items() if not v[0]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_rejection_is_the_parents(name, recorded):
    assert outcome(CASES[name]) == recorded[name]

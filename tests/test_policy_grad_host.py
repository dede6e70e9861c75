"""Host-side checks of the actor forward / backward in libuavx_actor.so (include/uavx_policy_grad.h): it builds for gfx950
without a GPU with the new translation unit under the source hash, it exports what its header declares, it rejects bad
arguments before touching a device, its workspace is what the header documents, its kernels neither spill nor use scratch,
the Python class refuses bad modules on the host, and the float64 formulas the GPU tests trust (tests/policy_grad_ref.py)
equal float64 autograd of the trainers' losses, kinks, clamps and the tie of torch.min included."""
import copy
import ctypes
import importlib.util
import json
import os
import re

import pytest
import torch

import policy_grad_ref as ref
from action_grad_ref import actor, actor_grads, actor_loss
from grad_ref import critic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["uavx_policy_grad_k::policy_bwd<false, 16>", "uavx_policy_grad_k::policy_bwd<true, 25>",
         "uavx_policy_grad_k::policy_combine", "uavx_policy_grad_k::policy_fwd<false, 16>",
         "uavx_policy_grad_k::policy_fwd<true, 25>"]


def _alib():
    from gym_uav_collision_avoidance_amd import _actor_lib
    _actor_lib.build()
    return _actor_lib


def _kernels():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr.kernel_table(_alib().LIB_PATH)


def test_policy_grad_library_cross_compiles_and_hash_covers_header():
    a = _alib()
    assert a.POLICY_GRAD_HEADER in a._sources()
    assert any(f.endswith("uavx_policy_grad.hip") for f in a._sources())
    assert f"UAVX_ACTOR_SRC_HASH={a.source_hash()}".encode() in open(a.LIB_PATH, "rb").read()
    mk = open(os.path.join(a.CSRC, "Makefile")).read()
    assert "uavx_policy_grad.hip" in mk and "uavx_policy_grad.h" in mk


def test_policy_grad_exports_every_declared_symbol():
    a = _alib()
    hdr = open(a.POLICY_GRAD_HEADER).read()
    declared = set(re.findall(r"\b(uavx_policy_grad[a-z_0-9]*)\s*\(", hdr))
    assert declared == set(a.POLICY_GRAD_SYMBOLS), declared ^ set(a.POLICY_GRAD_SYMBOLS)
    assert set(a.POLICY_GRAD_SYMBOLS).isdisjoint(a.SYMBOLS + a.CRITIC_SYMBOLS + a.GRAD_SYMBOLS + a.OPTIM_SYMBOLS
                                                 + a.REPLAY_SYMBOLS + a.ACTION_GRAD_SYMBOLS)
    lib = a.load()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.uavx_policy_grad_version() == a.POLICY_GRAD_ABI_VERSION == 1
    assert f"#define UAVX_POLICY_GRAD_MAX_ROWS {a.POLICY_GRAD_MAX_ROWS}" in hdr
    assert "#define UAVX_POLICY_GRAD_VERSION 1" in hdr


def _workspace(kind, h1, h2, rows):
    """The header's formula."""
    up = lambda x, m: -(-x // m) * m
    b16, n1, n2, O = up(rows, 16), up(h1, 16), up(h2, 16), 4 if kind == 0 else 2
    lp = up(11 * h1 + (1 + O) * h2 + O + 2, 4)
    tiles = -(-h2 // 64) * -(-h1 // 64)
    s0 = min(max(8192 // tiles, 1), -(-b16 // 64))
    kc = up(-(-b16 // s0), 16)
    S = -(-b16 // kc)
    regions = (b16 * n1 * 4, b16 * n2 * 4, b16 * 8 * 4, b16 // 16 * lp * 8, S * h2 * h1 * 4, S * lp * 8)
    return sum(up(r, 256) for r in regions)


def test_policy_grad_workspace_bytes_is_the_documented_formula():
    a = _alib()
    lib = a.load()
    n = ctypes.c_int64()
    for kind, h1, h2 in ((a.SAC, 256, 256), (a.TD3, 256, 256), (a.DDPG, 400, 300), (a.SAC, 241, 1), (a.TD3, 241, 1),
                         (a.DDPG, 385, 4096)):
        for rows in (1, 16, 17, 256, 262144):
            assert lib.uavx_policy_grad_workspace_bytes(kind, h1, h2, rows, ctypes.byref(n)) == a.OK
            assert n.value == _workspace(kind, h1, h2, rows), (kind, h1, h2, rows, n.value)
    assert _workspace(a.SAC, 256, 256, 256) == 256 * 256 * 4 * 2 + 256 * 32 + 16 * 4104 * 8 + 4 * (256 * 256 * 4 + 4104 * 8)
    # errors leave 0 behind
    n.value = 7
    assert lib.uavx_policy_grad_workspace_bytes(a.SAC, 256, 256, 0, ctypes.byref(n)) == a.ERR_INVALID_ARG and n.value == 0
    assert lib.uavx_policy_grad_workspace_bytes(a.SAC, 256, 256, a.POLICY_GRAD_MAX_ROWS + 1, ctypes.byref(n)) == a.ERR_INVALID_ARG
    assert lib.uavx_policy_grad_workspace_bytes(a.SAC, 128, 256, 16, ctypes.byref(n)) == a.ERR_UNSUPPORTED
    assert lib.uavx_policy_grad_workspace_bytes(a.DDPG, 256, 256, 16, ctypes.byref(n)) == a.ERR_UNSUPPORTED
    assert lib.uavx_policy_grad_workspace_bytes(a.TD3, 400, 300, 16, ctypes.byref(n)) == a.ERR_UNSUPPORTED
    assert lib.uavx_policy_grad_workspace_bytes(a.TD3, 256, 4097, 16, ctypes.byref(n)) == a.ERR_UNSUPPORTED
    assert lib.uavx_policy_grad_workspace_bytes(3, 256, 256, 16, ctypes.byref(n)) == a.ERR_INVALID_ARG
    assert lib.uavx_policy_grad_workspace_bytes(a.SAC, 256, 256, 16, None) == a.ERR_INVALID_ARG


def test_policy_grad_bad_arguments_rejected_before_any_device_call():
    a = _alib()
    lib = a.load()
    buf = ctypes.c_void_p(16)     # never dereferenced: every call that gets it fails its argument check first
    full = (ctypes.c_void_p * 8)(*([16] * 8))
    six = (ctypes.c_void_p * 8)(*([16] * 6 + [None] * 2))
    five = (ctypes.c_void_p * 8)(*([16] * 5 + [None] * 3))
    big = 1 << 40

    def fwd(kind=a.SAC, h1=256, h2=256, params=full, state=buf, rows=4, ss=10, eps=buf, action=buf, log_pi=buf, ws=buf,
            wsb=big):
        return lib.uavx_policy_grad_forward(kind, h1, h2, params, state, rows, ss, eps, action, log_pi, ws, wsb, None)

    def bwd(kind=a.SAC, h1=256, h2=256, params=full, state=buf, rows=4, ss=10, q=buf, dqda=buf, qts=4, grads=full,
            loss=buf, lpm=buf, ws=buf, wsb=big):
        return lib.uavx_policy_grad_backward(kind, h1, h2, params, state, rows, ss, q, dqda, qts, 0.2, None, grads, loss, lpm,
                                             ws, wsb, None)

    for call in (fwd, bwd):
        assert call(params=None) == a.ERR_INVALID_ARG          # NULL params
        assert call(state=None) == a.ERR_INVALID_ARG           # NULL state
        assert call(rows=0) == a.ERR_INVALID_ARG               # no rows
        assert call(rows=-3) == a.ERR_INVALID_ARG
        assert call(rows=a.POLICY_GRAD_MAX_ROWS + 1) == a.ERR_INVALID_ARG
        assert call(ss=9) == a.ERR_INVALID_ARG                 # short / negative strides
        assert call(ss=-10) == a.ERR_INVALID_ARG
        assert call(params=six) == a.ERR_INVALID_ARG           # SAC without W3b / b3b
        assert call(kind=a.TD3, params=five) == a.ERR_INVALID_ARG
        assert call(h1=128) == a.ERR_UNSUPPORTED               # no register tile of that width
        assert call(kind=a.DDPG, h1=256) == a.ERR_UNSUPPORTED
        assert call(kind=a.TD3, h1=400, h2=300) == a.ERR_UNSUPPORTED
        assert call(h2=4097) == a.ERR_UNSUPPORTED
        assert call(h2=0) == a.ERR_INVALID_ARG
        assert call(kind=3) == a.ERR_INVALID_ARG
        assert call(kind=-1) == a.ERR_INVALID_ARG
        assert call(ws=None) == a.ERR_INVALID_ARG
        assert call(ws=ctypes.c_void_p(20)) == a.ERR_INVALID_ARG                               # not 16-byte aligned
        for kind, h1, h2 in ((a.SAC, 256, 256), (a.TD3, 256, 256), (a.DDPG, 400, 300)):
            params = full if kind == a.SAC else six
            kw = dict(kind=kind, h1=h1, h2=h2, params=params)
            if call is bwd:
                kw["grads"] = params
            assert call(wsb=_workspace(kind, h1, h2, 4) - 1, **kw) == a.ERR_INVALID_ARG      # a short workspace
            assert call(wsb=0, **kw) == a.ERR_INVALID_ARG
            assert call(wsb=-1, **kw) == a.ERR_INVALID_ARG
    assert fwd(eps=None) == a.ERR_INVALID_ARG                  # SAC draws nothing itself
    assert fwd(log_pi=None) == a.ERR_INVALID_ARG
    assert fwd(action=None) == a.ERR_INVALID_ARG
    assert bwd(grads=None) == a.ERR_INVALID_ARG
    assert bwd(grads=six) == a.ERR_INVALID_ARG
    assert bwd(q=None) == a.ERR_INVALID_ARG
    assert bwd(dqda=None) == a.ERR_INVALID_ARG
    assert bwd(loss=None) == a.ERR_INVALID_ARG
    assert bwd(lpm=None) == a.ERR_INVALID_ARG
    assert bwd(qts=3) == a.ERR_INVALID_ARG                     # towers would overlap
    assert bwd(qts=-4) == a.ERR_INVALID_ARG


def test_policy_grad_kernels_no_spills_no_scratch():
    rows = _kernels()
    pg = [r for r in rows if r["name"].startswith("uavx_policy_grad_k::")]
    names = sorted(r["name"] for r in pg)
    assert names == NAMES, names
    for r in pg:
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["private_segment_fixed_size"] == 0, r
        assert r["max_flat_workgroup_size"] in (256, 512), r
        regs = r["vgpr_count"] + r["agpr_count"]
        assert regs <= (256 if r["max_flat_workgroup_size"] == 512 else 512), r    # the workgroup fits one CU
        assert r["group_segment_fixed_size"] <= 160 * 1024, r
    rec = {r["name"]: r for r in json.load(open(os.path.join(ROOT, "profiles", "r14_policy_grad_kernel_resources.json")))}
    assert set(rec) == set(names)
    for r in pg:
        for f in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "max_flat_workgroup_size"):
            assert rec[r["name"]][f] == r[f], (r["name"], f, rec[r["name"]][f], r[f])
    # the existing tiles keep their counts: nothing of the new unit is named like them, nothing of theirs changed
    assert sum(r["name"].startswith("uavx_critic_k::critic_fwd<") for r in rows) == 16
    assert sum(r["name"].startswith("uavx_critic_grad_k::") for r in rows) == 5      # grad_combine, and each tile of grad_rows unweighted and weighted
    assert sum(r["name"].startswith("uavx_action_grad_k::") for r in rows) == 2
    assert sum(r["name"].startswith("uavx_optim_k::") for r in rows) == 3


def test_python_policy_grad_api_rejects_bad_modules_before_the_device():
    from gym_uav_collision_avoidance_amd import policy
    from gym_uav_collision_avoidance_amd.fused_policy_grad import FusedPolicyGrad
    with pytest.raises(TypeError):
        FusedPolicyGrad(policy.TwinQ(), policy.TwinQ())                    # not an actor
    with pytest.raises(TypeError):
        FusedPolicyGrad(torch.nn.Linear(10, 2), policy.TwinQ())
    with pytest.raises(TypeError):
        FusedPolicyGrad(policy.TD3Actor(), policy.TD3Actor())              # not a critic
    with pytest.raises(TypeError):
        FusedPolicyGrad(policy.TD3Actor(), policy.TwinQ())                 # a TD3 actor with a SAC critic
    with pytest.raises(TypeError):
        FusedPolicyGrad(policy.GaussianPolicy(), policy.DDPGCritic())
    with pytest.raises(ValueError):
        FusedPolicyGrad(policy.TD3Actor(), policy.TD3TwinQ())              # CPU modules: no CPU path
    with pytest.raises(ValueError):
        FusedPolicyGrad(policy.GaussianPolicy(), policy.TwinQ())
    with pytest.raises(ValueError):
        FusedPolicyGrad(policy.DDPGActor(), policy.DDPGCritic())


def _kinked(kind, rows, seed):
    """An actor, a critic and a batch that sits ON the kinks: layer-1 biases 0 and the first rows' states 0 give z1 = 0
    exactly there; layer-2 biases <= 0, half of them 0, give z2 = 0 there (and, for relu, h2 = 0, so that the raw log-std of
    those rows is log_std_linear's bias exactly: 2.0 and -20.0, on both clamps); the widened log_std_linear puts the other
    rows' raw log-std on either side of both clamps.

    eps is 0 in a column whose log-std is below -8.  There autograd, the reference here, is itself inexact: the gradients of
    log N(x; mu, sigma) through x and through mu are -+eps / sigma each and cancel to their rounding, about
    2^-53 |eps| / sigma = 5e-8 |eps| at sigma = e^-20, times alpha / B: above 1e-9 of a mean_linear gradient of 1e-3 / B.
    With eps = 0 both terms are exactly 0, and the clamp's own gradient, -alpha / B, still passes through the mask."""
    pol, crit = actor(kind, seed), critic(kind, seed + 1)
    l1, l2 = ref.layers(kind, pol)[:2]
    with torch.no_grad():
        l1.bias.zero_()
        l2.bias.copy_(-l2.bias.abs())
        l2.bias[::2] = 0.0
        if kind == "sac":
            pol.log_std_linear.weight.mul_(30.0)
            pol.log_std_linear.bias.copy_(torch.tensor([2.0, -20.0]))
    g = torch.Generator().manual_seed(seed + rows)
    s = torch.randn((rows, 10), generator=g, dtype=torch.float64)
    s[:max(1, rows // 8)] = 0.0
    noise = torch.randn((rows, 2), generator=g, dtype=torch.float64) if kind == "sac" else None
    if kind == "sac":
        noise[ref.actor_preacts(kind, pol, s)[1] < -8.0] = 0.0
    return pol, crit, s, noise


@pytest.mark.parametrize("rows", [1, 17, 257])
@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_formulas_equal_float64_autograd(kind, rows):
    """Bound: 1e-9 of each tensor's maximum.  The formulas and autograd run the same float64 chain rule; autograd's own
    noise is largest on SAC's mean path, where the gradients of log N(x; mu, sigma) through x and through mu cancel
    (about 1e-11)."""
    pol, crit, s, noise = _kinked(kind, rows, seed=40)
    (z1, z2), raw = ref.actor_preacts(kind, pol, s)
    k = max(1, rows // 8)
    assert bool((z1[:k] == 0).all()) and bool((z2[:k, ::2] == 0).all())
    if kind == "sac":
        assert bool((raw[:k, 0] == 2.0).all()) and bool((raw[:k, 1] == -20.0).all())          # exactly on both clamps
        if rows > 1:
            for j, edge in ((0, 2.0), (1, -20.0)):
                assert bool((raw[k:, j] > edge).any()) and bool((raw[k:, j] < edge).any())    # and on either side
    g64, l64, p64 = actor_grads(kind, pol, crit, s, alpha=0.2, noise=noise)
    q, J = ref.critic_at(kind, pol, crit, s, noise)
    out = ref.analytic(kind, pol, s, q, J, alpha=0.2, noise=noise)
    assert len(out["grads"]) == len(g64) == (8 if kind == "sac" else 6)
    for i, (x, r) in enumerate(zip(out["grads"], g64)):
        assert x.shape == r.shape
        top = float(r.abs().max())                      # 0 for W1 when every state of the batch is 0: then equal
        assert float((x - r).abs().max()) <= 1e-9 * top, (i, float((x - r).abs().max()), top)
    assert abs(float(out["loss"]) - float(l64)) <= 1e-12 * abs(float(l64))
    if kind == "sac":
        assert float((out["log_pi"] - p64).abs().max()) <= 1e-12 * float(p64.abs().max())
        assert abs(float(out["log_pi_mean"]) - float(p64.mean())) <= 1e-12 * abs(float(p64.mean()))
        # the clamp passes its gradient AT equality: the zero rows alone give log_std_linear's bias a gradient
        o1 = ref.analytic(kind, pol, s[:k], q[:, :k], J[:, :k], alpha=0.2, noise=noise[:k])
        assert bool((o1["grads"][7] != 0).all())


class _Given(torch.autograd.Function):
    """A critic stand-in: returns the given q_t whatever the action and hands the given J_t back as dq_t/da."""

    @staticmethod
    def forward(ctx, a, q, J):
        ctx.J = J
        return tuple(x.unsqueeze(1).clone() for x in q)

    @staticmethod
    def backward(ctx, *gs):
        return sum(g * j for g, j in zip(gs, ctx.J)), None, None


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_tie_of_the_twin_minimum_splits_the_gradient(kind):
    """q and J given (random), q1 == q2 bitwise on a third of the rows with J1 != J2: autograd through torch.min of the
    stand-in gives each tower half, and so do the formulas; either one-sided choice is far outside the bound."""
    rows, T = 48, 1 if kind == "ddpg" else 2
    pol = actor(kind, 50)
    g = torch.Generator().manual_seed(51)
    s = torch.randn((rows, 10), generator=g, dtype=torch.float64)
    noise = torch.randn((rows, 2), generator=g, dtype=torch.float64) if kind == "sac" else None
    q = torch.randn((T, rows), generator=g, dtype=torch.float64)
    J = torch.randn((T, rows, 2), generator=g, dtype=torch.float64)
    if T == 2:
        q[1, ::3] = q[0, ::3]
    p64 = copy.deepcopy(pol).double()

    def fn(ss, aa):
        out = _Given.apply(aa, q, J)
        return out if T == 2 else out[0]

    loss, _ = actor_loss(kind, p64, fn, s, 0.2, noise)
    gs = torch.autograd.grad(loss, list(p64.parameters()))
    out = ref.analytic(kind, pol, s, q, J, alpha=0.2, noise=noise)
    for x, r in zip(out["grads"], gs):
        assert float((x - r).abs().max()) <= 1e-9 * float(r.abs().max())
    assert abs(float(out["loss"]) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    if kind == "sac":
        for tie in (0.0, 1.0):
            one = ref.analytic(kind, pol, s, q, J, alpha=0.2, noise=noise, tie=tie)
            assert max(float((x - r).abs().max()) / float(r.abs().max()) for x, r in zip(one["grads"], gs)) > 1e-3

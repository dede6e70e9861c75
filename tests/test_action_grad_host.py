"""Host-side checks of the critic action-gradient in libuavx_actor.so (include/uavx_action_grad.h): it builds for gfx950
without a GPU with the new translation unit under the source hash, it exports what its header declares, it rejects bad
arguments before touching a device, its kernels neither spill nor use scratch, the Python classes refuse bad modules on the
host, the float64 references the GPU tests trust agree with each other, and an autograd function that keeps the critic's
Jacobian reproduces the full-autograd actor gradient of all three learners (the seam FusedActorLoss is cut at)."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

from action_grad_ref import actor, actor_grads, analytic, jacobian, seam_critic
from grad_ref import critic, towers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _alib():
    from gym_uav_collision_avoidance_amd import _actor_lib
    _actor_lib.build()
    return _actor_lib


def _kernels():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr.kernel_table(_alib().LIB_PATH)


class _Layout(ctypes.Structure):
    """uavx_actor_k::Layout of actor_csrc/uavx_actor_impl.hpp."""
    _fields_ = ([(n, ctypes.c_int) for n in ("prec", "nb1", "nb2", "ks1", "ks2", "ks3", "epl")]
                + [(n, ctypes.c_int64) for n in ("b1", "b2", "b3", "w1", "w2", "w3", "bias_floats", "frag_elems")])


class _Handle(ctypes.Structure):
    """struct uavx_critic of actor_csrc/uavx_actor_impl.hpp: uavx_critic_create needs a device, so the checks that read a
    handle get a host-side one.  uavx_action_grad reads only the dimensions; the same checks run on real handles in
    tests/test_gpu_action_grad.py."""
    _fields_ = ([(n, ctypes.c_int) for n in ("kind", "prec", "h1", "h2", "towers")] + [("L", _Layout)]
                + [("bias", ctypes.c_void_p), ("frags", ctypes.c_void_p), ("split_rows", ctypes.c_int64),
                   ("packed", ctypes.c_bool)])


def _handle(a, kind, prec=0):
    h = _Handle()
    h.kind, h.prec, h.towers = kind, prec, 1 if kind == a.DDPG else 2
    h.h1, h.h2 = (400, 300) if kind == a.DDPG else (256, 256)
    h.L.prec, h.L.nb1, h.L.nb2 = prec, (h.h1 + 15) // 16, (h.h2 + 15) // 16
    return h


def test_action_grad_library_cross_compiles_and_hash_covers_header():
    a = _alib()
    assert a.ACTION_GRAD_HEADER in a._sources()
    assert any(f.endswith("uavx_action_grad.hip") for f in a._sources())
    assert f"UAVX_ACTOR_SRC_HASH={a.source_hash()}".encode() in open(a.LIB_PATH, "rb").read()
    mk = open(os.path.join(a.CSRC, "Makefile")).read()
    assert "uavx_action_grad.hip" in mk and "uavx_action_grad.h" in mk


def test_action_grad_exports_every_declared_symbol():
    a = _alib()
    hdr = open(a.ACTION_GRAD_HEADER).read()
    declared = set(re.findall(r"\b(uavx_action_grad[a-z_0-9]*)\s*\(", hdr))
    assert declared == set(a.ACTION_GRAD_SYMBOLS), declared ^ set(a.ACTION_GRAD_SYMBOLS)
    assert set(a.ACTION_GRAD_SYMBOLS).isdisjoint(a.SYMBOLS + a.CRITIC_SYMBOLS + a.GRAD_SYMBOLS + a.OPTIM_SYMBOLS
                                                 + a.REPLAY_SYMBOLS)
    lib = a.load()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.uavx_action_grad_version() == a.ACTION_GRAD_ABI_VERSION == 1
    assert f"#define UAVX_ACTION_GRAD_MAX_ROWS {a.ACTION_GRAD_MAX_ROWS}" in hdr
    assert "#define UAVX_ACTION_GRAD_VERSION 1" in hdr


def test_action_grad_bad_arguments_rejected_before_any_device_call():
    a = _alib()
    lib = a.load()
    buf = ctypes.c_void_p(16)     # never dereferenced: every call that gets it fails its argument check first
    ptrs = (ctypes.c_void_p * 12)(*([16] * 12))
    twin, ddpg, bf16 = _handle(a, a.SAC), _handle(a, a.DDPG), _handle(a, a.TD3, prec=a.BF16)

    def call(h=buf, mask=1, params=ptrs, rows=4, ss=10, as_=2, q=buf, dqda=buf):
        h = ctypes.byref(h) if isinstance(h, _Handle) else h
        return lib.uavx_action_grad(h, mask, params, buf, rows, ss, buf, as_, q, dqda, None)

    assert call(h=None) == a.ERR_INVALID_ARG               # NULL handle
    assert call(params=None) == a.ERR_INVALID_ARG          # NULL params
    assert call(dqda=None) == a.ERR_INVALID_ARG            # NULL dqda (q alone may be NULL)
    assert call(rows=0) == a.ERR_INVALID_ARG               # no rows
    assert call(rows=-3) == a.ERR_INVALID_ARG
    assert call(rows=a.ACTION_GRAD_MAX_ROWS + 1) == a.ERR_INVALID_ARG
    assert call(ss=9) == a.ERR_INVALID_ARG                 # short / negative strides
    assert call(ss=-10) == a.ERR_INVALID_ARG
    assert call(as_=1) == a.ERR_INVALID_ARG
    assert call(as_=-2) == a.ERR_INVALID_ARG
    for h in (buf, twin, ddpg):
        assert call(h=h, mask=0) == a.ERR_INVALID_ARG      # selects nothing
        assert call(h=h, mask=4) == a.ERR_INVALID_ARG
        assert call(h=h, mask=-1) == a.ERR_INVALID_ARG
    assert call(h=ddpg, mask=2) == a.ERR_INVALID_ARG       # a tower the DDPG handle does not have
    assert call(h=ddpg, mask=3) == a.ERR_INVALID_ARG
    for mask in (1, 2, 3):
        assert call(h=bf16, mask=mask) == a.ERR_UNSUPPORTED
    # a selected tower's parameter pointer missing (DDPG passes six, then NULLs: tower 2 of a twin needs its own)
    half = (ctypes.c_void_p * 12)(*([16] * 6 + [None] * 6))
    assert call(h=twin, mask=2, params=half) == a.ERR_INVALID_ARG
    assert call(h=twin, mask=3, params=half) == a.ERR_INVALID_ARG
    none = (ctypes.c_void_p * 12)()
    assert call(h=ddpg, mask=1, params=none) == a.ERR_INVALID_ARG


def test_action_grad_kernels_no_spills_no_scratch():
    rows = _kernels()
    ag = [r for r in rows if r["name"].startswith("uavx_action_grad_k::")]
    names = sorted(r["name"] for r in ag)
    assert names == ["uavx_action_grad_k::action_grad<false, 16>", "uavx_action_grad_k::action_grad<true, 25>"], names
    for r in ag:
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["private_segment_fixed_size"] == 0, r
        assert r["max_flat_workgroup_size"] == 512, r
        assert r["vgpr_count"] + r["agpr_count"] <= 256, r           # 8 waves of one workgroup on a CU: 2 per SIMD
        assert r["group_segment_fixed_size"] <= 160 * 1024, r
    rec = {r["name"]: r for r in __import__("json").load(open(os.path.join(ROOT, "profiles",
                                                                          "r13_action_grad_kernel_resources.json")))}
    assert set(rec) == set(names)
    # the existing tiles keep their counts: nothing of the new unit is named like them
    assert sum(r["name"].startswith("uavx_critic_k::critic_fwd<") for r in rows) == 16
    assert sum(r["name"].startswith("uavx_critic_grad_k::") for r in rows) == 5      # grad_combine, and each tile of grad_rows unweighted and weighted


def test_python_action_grad_api_rejects_bad_modules_before_the_device():
    from gym_uav_collision_avoidance_amd import policy
    from gym_uav_collision_avoidance_amd.fused_critic import FusedActionGrad, FusedActorLoss
    with pytest.raises(TypeError):
        FusedActionGrad(policy.TD3Actor())                       # not a critic
    with pytest.raises(TypeError):
        FusedActionGrad(torch.nn.Linear(12, 1))
    with pytest.raises(ValueError):
        FusedActionGrad(policy.TwinQ())                          # CPU parameters: no CPU path
    with pytest.raises(TypeError):
        FusedActorLoss(policy.TwinQ(), policy.TwinQ())           # not an actor
    with pytest.raises(ValueError):
        FusedActorLoss(policy.TD3Actor(), policy.TD3TwinQ())     # CPU critic


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_float64_references_agree(kind):
    """autograd.grad with respect to the action against the formulas of the header written out, both in float64 on CPU
    (the full layer sizes, nonzero biases, rows and units at the activation kinks included)."""
    m = critic(kind, 3).double()
    g = torch.Generator().manual_seed(1)
    B = 37
    s = torch.randn((B, 10), generator=g, dtype=torch.float64)
    a = torch.rand((B, 2), generator=g, dtype=torch.float64) * 2 - 1
    s[:3] = 0.0                                        # z1 = b1 exactly on these rows
    a[:3] = 0.0
    with torch.no_grad():
        for t in towers(m):
            t[1][:40] = 0.0                            # z1 = 0 exactly on 40 units of those rows
    qa, ja = analytic(m, s, a)
    qt, jt = jacobian(m, s, a)
    assert len(qa) == len(qt) == (1 if kind == "ddpg" else 2)
    for x, r in zip(qa + ja, qt + jt):
        assert x.shape == r.shape
        assert float((x - r).abs().max()) <= 1e-12, float((x - r).abs().max())
    # the convention at the kink matters on these rows: a slope of 1 at z = 0 gives another Jacobian
    _, jk = analytic(m, s, a, kink_slope=1.0)
    assert max(float((x - r).abs().max()) for x, r in zip(jk, jt)) > 1e-6


@pytest.mark.parametrize("rows", [1, 17, 257])
@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_seam_reproduces_the_full_autograd_actor_gradient(kind, rows):
    """The actor gradient through an autograd function that returns q and keeps J (backward: sum_t g_t * J_t) equals the
    one through the critic module's own graph, in float64: both are the chain rule through the same dq/da, so they differ
    by rounding only (bound: 1e-12 of the largest entry, about 1e4 ulp for sums of up to 257 x 256 terms)."""
    pol, crit = actor(kind, 5), critic(kind, 6)
    g = torch.Generator().manual_seed(rows)
    s = torch.randn((rows, 10), generator=g, dtype=torch.float64)
    noise = torch.randn((rows, 2), generator=g, dtype=torch.float64) if kind == "sac" else None
    full, lf, pf = actor_grads(kind, pol, crit, s, alpha=0.2, noise=noise)
    seam, ls, ps = actor_grads(kind, pol, crit, s, alpha=0.2, noise=noise, critic_fn=seam_critic)
    assert len(full) == len(seam) == len(list(pol.parameters()))
    for x, r in zip(seam, full):
        assert float((x - r).abs().max()) <= 1e-12 * float(r.abs().max()), (float((x - r).abs().max()), float(r.abs().max()))
    assert abs(float(ls) - float(lf)) <= 1e-12 * abs(float(lf))
    if kind == "sac":
        assert torch.equal(ps, pf)

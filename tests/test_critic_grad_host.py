"""Host-side checks of the critic-loss gradient in libuavx_actor.so (include/uavx_critic_grad.h): it builds for gfx950
without a GPU with the new translation unit under the source hash, it exports what its header declares, it rejects bad
arguments before touching a device, its kernels neither spill nor use scratch, the Python class refuses bad modules on the
host, and the float64 analytic backward the GPU tests trust equals torch.autograd."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

from grad_ref import analytic, autograd, critic

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


def test_grad_library_cross_compiles_and_hash_covers_header():
    a = _alib()
    assert a.GRAD_HEADER in a._sources()
    assert any(f.endswith("uavx_critic_grad.hip") for f in a._sources())
    assert f"UAVX_ACTOR_SRC_HASH={a.source_hash()}".encode() in open(a.LIB_PATH, "rb").read()
    mk = open(os.path.join(a.CSRC, "Makefile")).read()
    assert "uavx_critic_grad.hip" in mk and "uavx_critic_grad.h" in mk


def test_grad_exports_every_declared_symbol():
    a = _alib()
    hdr = open(a.GRAD_HEADER).read()
    declared = set(re.findall(r"\b(uavx_critic_grad[a-z_0-9]*)\s*\(", hdr))
    assert declared == set(a.GRAD_SYMBOLS), declared ^ set(a.GRAD_SYMBOLS)
    assert set(a.GRAD_SYMBOLS).isdisjoint(a.SYMBOLS + a.CRITIC_SYMBOLS)
    lib = a.load()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.uavx_critic_grad_version() == 1
    assert f"#define UAVX_CRITIC_GRAD_MAX_ROWS {a.GRAD_MAX_ROWS}" in hdr
    assert "UAVX_CRITIC_GRAD_MSE = 0" in hdr and "UAVX_CRITIC_GRAD_L1 = 1" in hdr


def test_grad_bad_arguments_rejected_before_any_device_call():
    a = _alib()
    lib = a.load()
    buf = ctypes.c_void_p(16)     # never dereferenced: every call below fails its argument check first
    ptrs = (ctypes.c_void_p * 12)(*([16] * 12))
    n = ctypes.c_int64(7)
    assert lib.uavx_critic_grad_workspace_bytes(None, 256, ctypes.byref(n)) == a.ERR_INVALID_ARG
    assert n.value == 0
    assert lib.uavx_critic_grad_workspace_bytes(buf, 256, None) == a.ERR_INVALID_ARG

    def call(h=None, loss=a.GRAD_MSE, rows=4, ss=10, as_=2, ys=1):
        return lib.uavx_critic_grad(h, loss, ptrs, buf, rows, ss, buf, as_, buf, ys, ptrs, buf, buf, 1 << 30, None)

    assert call() == a.ERR_INVALID_ARG                     # NULL handle
    assert call(buf, rows=0) == a.ERR_INVALID_ARG          # no rows
    assert call(buf, rows=-3) == a.ERR_INVALID_ARG
    assert call(buf, ss=-10) == a.ERR_INVALID_ARG          # negative / short strides
    assert call(buf, ss=9) == a.ERR_INVALID_ARG
    assert call(buf, as_=-2) == a.ERR_INVALID_ARG
    assert call(buf, ys=-1) == a.ERR_INVALID_ARG
    assert call(buf, ys=0) == a.ERR_INVALID_ARG
    assert call(buf, loss=2) == a.ERR_INVALID_ARG          # unknown loss
    assert call(buf, loss=-1) == a.ERR_INVALID_ARG
    assert lib.uavx_critic_grad(buf, 0, None, buf, 4, 10, buf, 2, buf, 1, ptrs, buf, buf, 1 << 30, None) == a.ERR_INVALID_ARG
    assert lib.uavx_critic_grad(buf, 0, ptrs, buf, 4, 10, buf, 2, buf, 1, None, buf, buf, 1 << 30, None) == a.ERR_INVALID_ARG


def test_grad_kernels_no_spills_no_scratch():
    rows = _kernels()
    grad = [r for r in rows if r["name"].startswith("uavx_critic_grad_k::")]
    names = sorted(r["name"] for r in grad)
    # each tile of the row pass twice: the unweighted call's and the weighted one's (include/uavx_wcritic_grad.h)
    assert names == ["uavx_critic_grad_k::grad_combine", "uavx_critic_grad_k::grad_rows<false, 16, false>",
                     "uavx_critic_grad_k::grad_rows<false, 16, true>", "uavx_critic_grad_k::grad_rows<true, 25, false>",
                     "uavx_critic_grad_k::grad_rows<true, 25, true>"], names
    # the dW2 weights kernel this unit shares with the actor backward (actor_csrc/uavx_grad_common.hip)
    shared = [r for r in rows if r["name"].startswith("uavx_grad_k::")]
    assert [r["name"] for r in shared] == ["uavx_grad_k::grad_weights"], shared
    for r in shared:
        assert r["group_segment_fixed_size"] == 0, r
        # what grad_weights and policy_weights each used before they became one kernel.  vgpr_count is the unified
        # register file's total (.amdhsa_next_free_vgpr): the 64 accumulator registers of the 4 x 4 tile are part of it
        assert r["vgpr_count"] <= 92 and r["agpr_count"] <= 64, r
    for r in grad + shared:
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["private_segment_fixed_size"] == 0, r
        assert r["max_flat_workgroup_size"] == 256, r
        assert r["group_segment_fixed_size"] <= 160 * 1024, r
    # the existing tiles keep their counts: nothing of the new unit is named like them
    assert sum(r["name"].startswith("uavx_critic_k::critic_fwd<") for r in rows) == 16


def test_grad_source_has_no_scalar_memory_writes():
    a = _alib()
    src = open(os.path.join(a.CSRC, "uavx_critic_grad.hip")).read() + open(a.GRAD_HEADER).read()
    assert not re.search(r"s_(buffer_|scratch_)?(store|atomic)|s_dcache", src, re.I)


def test_python_grad_api_rejects_bad_modules_before_the_device():
    from gym_uav_collision_avoidance_amd import policy
    from gym_uav_collision_avoidance_amd.fused_critic import FusedCriticLoss
    with pytest.raises(TypeError):
        FusedCriticLoss(policy.TD3Actor())                       # not a critic
    with pytest.raises(TypeError):
        FusedCriticLoss(torch.nn.Linear(12, 1))
    with pytest.raises(ValueError):
        FusedCriticLoss(policy.TwinQ(), loss="huber")            # unknown loss, before any device work
    with pytest.raises(ValueError):
        FusedCriticLoss(policy.TwinQ())                          # CPU parameters: no CPU path
    with pytest.raises(ValueError):
        FusedCriticLoss(policy.DDPGCritic(), loss="l1")


@pytest.mark.parametrize("loss", ["mse", "l1"])
@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_float64_reference_equals_autograd(kind, loss):
    """The analytic backward of grad_ref.py against torch.autograd, both in float64 on CPU (small layers, nonzero biases,
    rows at the activation kinks included)."""
    m = critic(kind, 3, hidden1=24 if kind != "ddpg" else 40, hidden2=17).double()
    g = torch.Generator().manual_seed(1)
    B = 37
    s = torch.randn((B, 10), generator=g, dtype=torch.float64)
    a = torch.rand((B, 2), generator=g, dtype=torch.float64) * 2 - 1
    y = torch.randn((B,), generator=g, dtype=torch.float64)
    s[:3] = 0.0                                        # z1 = b1 exactly on these rows
    a[:3] = 0.0
    with torch.no_grad():
        from grad_ref import towers
        for t in towers(m):
            t[1][:5] = 0.0                             # and z1 = 0 exactly on 5 units
    ga, la = analytic(m, s, a, y, loss)
    gt, lt = autograd(m, s, a, y, loss)
    assert len(ga) == len(gt) == (6 if kind == "ddpg" else 12)
    for x, r in zip(ga, gt):
        assert x.shape == r.shape
        assert torch.allclose(x, r, rtol=1e-12, atol=1e-14), float((x - r).abs().max())
    for x, r in zip(la, lt):
        assert abs(float(x) - float(r)) <= 1e-12 * abs(float(r))
    # the convention at the kink matters on these rows: a slope of 1 at z = 0 gives other gradients
    gk, _ = analytic(m, s, a, y, loss, kink_slope=1.0)
    assert max(float((x - r).abs().max()) for x, r in zip(gk, gt)) > 1e-6

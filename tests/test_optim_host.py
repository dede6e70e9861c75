"""Host-side checks of the Adam step and soft update in libuavx_actor.so (include/uavx_optim.h): the library builds for
gfx950 without a GPU with the new translation unit under the source hash, exports what its header declares, rejects bad
arguments before touching a device, its kernels use no spills, scratch or LDS, FusedAdam refuses on the host what the
kernels do not implement, and the float64 reference the GPU tests trust equals torch.optim.Adam in float64."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

import optim_ref

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


def test_optim_library_cross_compiles_and_hash_covers_header():
    a = _alib()
    assert a.OPTIM_HEADER in a._sources()
    assert any(f.endswith("uavx_optim.hip") for f in a._sources())
    assert f"UAVX_ACTOR_SRC_HASH={a.source_hash()}".encode() in open(a.LIB_PATH, "rb").read()
    mk = open(os.path.join(a.CSRC, "Makefile")).read()
    assert "uavx_optim.hip" in mk and "uavx_optim.h" in mk


def test_optim_exports_every_declared_symbol():
    a = _alib()
    hdr = open(a.OPTIM_HEADER).read()
    declared = set(re.findall(r"\b(uavx_optim_[a-z_0-9]*)\s*\(", hdr))
    assert declared == set(a.OPTIM_SYMBOLS), declared ^ set(a.OPTIM_SYMBOLS)
    assert set(a.OPTIM_SYMBOLS).isdisjoint(a.SYMBOLS + a.CRITIC_SYMBOLS + a.GRAD_SYMBOLS)
    lib = a.load()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.uavx_optim_version() == a.OPTIM_ABI_VERSION == 1
    assert f"#define UAVX_OPTIM_MAX_TENSORS {a.OPTIM_MAX_TENSORS}" in hdr
    from gym_uav_collision_avoidance_amd import fused_optim
    assert callable(fused_optim.FusedAdam) and callable(fused_optim.soft_update)


def test_optim_bad_arguments_rejected_before_any_device_call():
    a = _alib()
    lib = a.load()
    buf = ctypes.c_void_p(64)     # never dereferenced: every call below fails its argument check first
    ptrs = (ctypes.c_void_p * 17)(*([64] * 17))
    holes = (ctypes.c_void_p * 17)(*([64] * 5 + [None] + [64] * 11))
    odd = (ctypes.c_void_p * 17)(*([64] * 5 + [66] + [64] * 11))
    num = (ctypes.c_int64 * 17)(*([8] * 17))

    def adam(n=12, p=ptrs, g=ptrs, m=ptrs, v=ptrs, x=None, t=None, numel=num, lr=3e-4, b1=0.9, b2=0.999, eps=1e-8, tau=5e-3,
             step=buf, scal=buf):
        return lib.uavx_optim_adam(n, p, g, m, v, x, t, numel, lr, b1, b2, eps, tau, step, scal, None)

    bad = a.ERR_INVALID_ARG
    assert adam(n=0) == bad and adam(n=-1) == bad and adam(n=17) == bad
    assert adam(p=None) == bad and adam(g=None) == bad and adam(m=None) == bad and adam(v=None) == bad
    assert adam(numel=None) == bad
    assert adam(p=holes) == bad and adam(g=holes) == bad and adam(m=holes) == bad and adam(v=holes) == bad
    assert adam(x=holes) == bad                                   # AMSGrad wants every tensor's max_exp_avg_sq
    assert adam(p=odd) == bad and adam(t=odd) == bad              # not 4-byte aligned
    for count in (0, -5, 2**31):
        assert adam(numel=(ctypes.c_int64 * 17)(*([8] * 3 + [count] + [8] * 13))) == bad
    assert adam(step=None) == bad and adam(scal=None) == bad
    assert adam(step=ctypes.c_void_p(68)) == bad and adam(scal=ctypes.c_void_p(68)) == bad
    nan, inf = float("nan"), float("inf")
    for kw in (dict(lr=-1e-3), dict(lr=nan), dict(lr=inf), dict(eps=-1e-8), dict(eps=nan), dict(b1=1.0), dict(b1=-0.1),
               dict(b1=nan), dict(b2=1.0), dict(b2=-0.1), dict(b2=nan)):
        assert adam(**kw) == bad, kw
    for tau in (-0.1, 1.5, nan):
        assert adam(t=ptrs, tau=tau) == bad, tau

    def soft(n=12, t=ptrs, s=ptrs, numel=num, tau=5e-3):
        return lib.uavx_optim_soft_update(n, t, s, numel, tau, None)

    assert soft(n=0) == bad and soft(n=17) == bad and soft(n=-2) == bad
    assert soft(t=None) == bad and soft(s=None) == bad and soft(numel=None) == bad
    assert soft(t=holes) == bad and soft(s=holes) == bad and soft(t=odd) == bad and soft(s=odd) == bad
    assert soft(numel=(ctypes.c_int64 * 17)(*([0] * 17))) == bad
    assert soft(numel=(ctypes.c_int64 * 17)(*([2**31] * 17))) == bad
    for tau in (-0.1, 1.5, nan):
        assert soft(tau=tau) == bad, tau


def test_optim_kernels_no_spills_no_scratch_no_lds():
    rows = _kernels()
    mine = [r for r in rows if r["name"].startswith("uavx_optim_k::")]
    names = sorted(r["name"] for r in mine)
    assert names == ["uavx_optim_k::adam_prologue", "uavx_optim_k::update<false>", "uavx_optim_k::update<true>"], names
    for r in mine:
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["private_segment_fixed_size"] == 0, r
        assert r["group_segment_fixed_size"] == 0, r
        assert r["agpr_count"] == 0 and r["vgpr_count"] <= 64, r         # 8 waves per SIMD
    # nothing of the new unit is counted among the pinned namespaces
    assert sum(r["name"].startswith("uavx_critic_grad_k::") for r in rows) == 5      # grad_combine, and each tile of grad_rows unweighted and weighted


def test_optim_source_has_no_scalar_memory_writes():
    a = _alib()
    src = open(os.path.join(a.CSRC, "uavx_optim.hip")).read() + open(a.OPTIM_HEADER).read()
    assert not re.search(r"s_(buffer_|scratch_)?(store|atomic)|s_dcache", src, re.I)
    assert "atomic" not in src.replace("no atomics", "")


def _cpu_adam(n=1, **kw):
    ps = [torch.nn.Parameter(torch.ones(3)) for _ in range(n)]
    return ps, torch.optim.Adam(ps, **kw)


def test_fused_adam_refuses_on_the_host():
    from gym_uav_collision_avoidance_amd.fused_optim import FusedAdam, soft_update
    ps = [torch.nn.Parameter(torch.ones(3))]
    for other in (torch.optim.AdamW(ps), torch.optim.SGD(ps, lr=0.1), torch.optim.Adamax(ps), object()):
        with pytest.raises(TypeError, match="uavx: FusedAdam wraps a torch.optim.Adam"):
            FusedAdam(other)
    with pytest.raises(ValueError, match="uavx: .*weight_decay"):
        FusedAdam(_cpu_adam(weight_decay=1e-2)[1])
    with pytest.raises(ValueError, match="uavx: .*maximize"):
        FusedAdam(_cpu_adam(maximize=True)[1])
    with pytest.raises(ValueError, match="uavx: .*differentiable"):
        FusedAdam(_cpu_adam(differentiable=True)[1])
    with pytest.raises(TypeError, match="uavx: .*float lr"):
        FusedAdam(_cpu_adam(lr=torch.tensor(1e-3))[1])
    with pytest.raises(ValueError, match="uavx: .*17 tensors"):
        FusedAdam(_cpu_adam(17)[1])
    with pytest.raises(ValueError, match="uavx: tau"):
        FusedAdam(_cpu_adam()[1], tau=1.5)
    with pytest.raises(ValueError, match="uavx: target has 2 parameters"):
        FusedAdam(_cpu_adam()[1], target=[torch.ones(3), torch.ones(3)])
    with pytest.raises(ValueError, match=r"uavx: target parameter 0 is \(4,\)"):
        FusedAdam(_cpu_adam()[1], target=[torch.ones(4)])
    with pytest.raises(ValueError, match="uavx: .*no CPU path"):
        FusedAdam(_cpu_adam()[1])                                    # CPU parameters
    p64 = [torch.nn.Parameter(torch.ones(3, dtype=torch.float64))]
    with pytest.raises(TypeError, match="uavx: .*float32"):
        FusedAdam(torch.optim.Adam(p64))
    with pytest.raises(ValueError, match="uavx: .*no CPU path"):
        soft_update([torch.ones(3)], [torch.ones(3)], 5e-3)
    with pytest.raises(ValueError, match="uavx: target has 1 parameters"):
        soft_update([torch.ones(3)], [torch.ones(3), torch.ones(3)], 5e-3)
    with pytest.raises(ValueError, match="uavx: tau"):
        soft_update([torch.ones(3)], [torch.ones(3)], -0.5)
    with pytest.raises(TypeError, match="uavx: .*float32"):
        soft_update([torch.ones(3, dtype=torch.float64)], [torch.ones(3, dtype=torch.float64)], 5e-3)


@pytest.mark.parametrize("amsgrad", [False, True])
def test_float64_reference_equals_torch_adam(amsgrad):
    """optim_ref in float64 against torch.optim.Adam on float64 CPU parameters over 200 steps of seeded gradients (lr 3e-4,
    gradients of scale 1e-2, four small tensors).  Bound 1e-13 of the largest parameter: a float64 ulp is 1.1e-16, the two
    differ by one or two of them; float32 rounding is 6e-8, so a wrong formula cannot pass."""
    g = torch.Generator().manual_seed(3)
    shapes = [(16, 12), (16,), (7, 16), (1,)]
    p0 = [torch.randn(s, generator=g, dtype=torch.float64) * 0.1 for s in shapes]
    grads = [[torch.randn(s, generator=g, dtype=torch.float64) * 1e-2 for s in shapes] for _ in range(200)]
    ps = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = torch.optim.Adam(ps, lr=3e-4, amsgrad=amsgrad)
    for gs in grads:
        for p, gr in zip(ps, gs):
            p.grad = gr.clone()
        opt.step()
    rp, rm, rv, rx = optim_ref.run(p0, grads, amsgrad, lr=3e-4)
    scale = max(float(p.detach().abs().max()) for p in ps)
    worst = max(float((p.detach() - r).abs().max()) for p, r in zip(ps, rp))
    print(f"amsgrad={amsgrad}: max |torch - ref| = {worst:.3e}, {worst / scale:.3e} of the largest parameter")
    assert worst <= 1e-13 * scale, (worst, scale)
    for p, m, v, x in zip(ps, rm, rv, rx):
        st = opt.state[p]
        assert float((st["exp_avg"] - m).abs().max()) <= 1e-13 * float(m.abs().max())
        assert float((st["exp_avg_sq"] - v).abs().max()) <= 1e-13 * float(v.abs().max())
        if amsgrad:
            assert float((st["max_exp_avg_sq"] - x).abs().max()) <= 1e-13 * float(x.abs().max())

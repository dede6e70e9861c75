"""Host-side checks of gradient-norm clipping (libuavx_clip.so, include/uavx_clip.h): the float64 restatement
the GPU tests trust (clip_ref.py) equals torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on float64 CPU parameters, its
float32 coefficient equals torch's float32 clamp bit for bit, the library builds for gfx950 without a GPU, carries its source
hash, exports exactly what its header declares, refuses every bad argument before touching a device, its kernels use no
scratch and spill nothing, and a FusedAdam built without max_grad_norm never imports the binding."""
import ctypes
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import clip_ref
import optim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _xlib():
    from gym_uav_collision_avoidance_amd import _clip_lib
    _clip_lib.build()
    return _clip_lib


def _kernels():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr.kernel_table(_xlib().LIB_PATH)


# ---- the restatement -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("case", ["active", "inactive", "at_the_norm"])
def test_float64_reference_equals_torch_clip_and_adam(case, amsgrad):
    """clip_ref + optim_ref in float64 against clip_grad_norm_ + torch.optim.Adam on float64 CPU parameters over 50 steps of
    seeded gradients.  Bound 1e-13 of the largest value, test_optim_host.py's for the same comparison without the clip: the
    two differ by a few float64 ulps (1.1e-16); float32 rounding is 6e-8, so a wrong formula cannot pass.
    active: the bound is a third of the typical norm; inactive: a hundred times it; at_the_norm: every step's bound is
    that step's own norm, where the coefficient is max_norm / (max_norm + 1e-6), just below 1."""
    g = torch.Generator().manual_seed(5)
    shapes = [(16, 12), (16,), (7, 16), (1,)]
    steps = 50
    p0 = [torch.randn(s, generator=g, dtype=torch.float64) * 0.1 for s in shapes]
    grads = [[torch.randn(s, generator=g, dtype=torch.float64) * 1e-2 for s in shapes] for _ in range(steps)]
    typical = clip_ref.norm64(grads[0])
    ps = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = torch.optim.Adam(ps, lr=3e-4, amsgrad=amsgrad)
    rp = [p.clone() for p in p0]
    rm, rv = [torch.zeros_like(p) for p in p0], [torch.zeros_like(p) for p in p0]
    rx = [torch.zeros_like(p) for p in p0] if amsgrad else None
    active = 0
    for k, gs in enumerate(grads):
        bound = {"active": typical / 3, "inactive": typical * 100, "at_the_norm": clip_ref.norm64(gs)}[case]
        for p, gr in zip(ps, gs):
            p.grad = gr.clone()
        total = torch.nn.utils.clip_grad_norm_(ps, bound)
        opt.step()
        rp, rm, rv, rx, norm, coef = clip_ref.clipped_step(rp, gs, rm, rv, rx, k + 1, bound)
        assert abs(float(total) - norm) <= 1e-13 * norm
        active += coef < 1.0
        for p, gr in zip(ps, gs):                     # clip_grad_norm_ rewrote .grad: g * coef
            assert float((p.grad - gr * coef).abs().max()) <= 1e-13 * float(gr.abs().max())
    assert active == {"active": steps, "inactive": 0, "at_the_norm": steps}[case]
    scale = max(float(p.detach().abs().max()) for p in ps)
    worst = max(float((p.detach() - r).abs().max()) for p, r in zip(ps, rp))
    print(f"{case} amsgrad={amsgrad}: max |torch - ref| = {worst:.3e}, {worst / scale:.3e} of the largest parameter")
    assert worst <= 1e-13 * scale, (worst, scale)
    for i, p in enumerate(ps):
        st = opt.state[p]
        assert float((st["exp_avg"] - rm[i]).abs().max()) <= 1e-13 * float(rm[i].abs().max())
        assert float((st["exp_avg_sq"] - rv[i]).abs().max()) <= 1e-13 * float(rv[i].abs().max())
        if amsgrad:
            assert float((st["max_exp_avg_sq"] - rx[i]).abs().max()) <= 1e-13 * float(rx[i].abs().max())


@pytest.mark.parametrize("max_norm", [1.0, 0.5, 10.0, 3e-3, 1e30])
def test_float32_coefficient_equals_torch_clamp_bit_for_bit(max_norm):
    m32 = np.float32(max_norm)
    norms = [np.float32(0.0), np.float32(1e-7), np.nextafter(m32, np.float32(0)), m32, np.nextafter(m32, np.float32(np.inf)),
             np.float32(1e30), np.float32(np.inf), np.float32(np.nan)]
    for norm in norms:
        want = torch.clamp(torch.tensor(float(m32), dtype=torch.float32) / (torch.tensor(float(norm), dtype=torch.float32) + 1e-6),
                           max=1.0)
        got = clip_ref.coef32(norm, max_norm)
        assert got.dtype == np.float32
        if np.isnan(norm):
            assert np.isnan(got) and bool(torch.isnan(want))
        else:
            assert got.view(np.int32) == want.numpy().view(np.int32), (norm, got, float(want))
    assert clip_ref.coef32(np.float32(np.inf), max_norm) == 0.0 and clip_ref.coef32(np.float32(0), max_norm) == 1.0
    # norm == max_norm still clips, by the 1e-6, wherever float32 can tell max_norm + 1e-6 from max_norm (half an ulp of
    # max_norm below 1e-6: max_norm < 16)
    assert (clip_ref.coef32(m32, max_norm) < 1.0) == (max_norm < 16)


# ---- the library -----------------------------------------------------------------------------------------------------------

def test_library_cross_compiles_and_carries_its_source_hash():
    x = _xlib()
    assert os.path.basename(x.LIB_PATH) == "libuavx_clip.so" and os.path.isfile(x.LIB_PATH)
    assert x.HEADER == os.path.join(ROOT, "include", "uavx_clip.h") and x.HEADER in x._sources()
    assert any(f.endswith(os.path.join("clip_csrc", "uavx_clip.hip")) for f in x._sources())
    blob = open(x.LIB_PATH, "rb").read()
    assert f"UAVX_CLIP_SRC_HASH={x.source_hash()}".encode() + b"\0" in blob and b"gfx950" in blob
    assert x._up_to_date()
    mk = open(os.path.join(x.CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, re.M).group(1)
    actor_mk = open(os.path.join(ROOT, "gym_uav_collision_avoidance_amd", "actor_csrc", "Makefile")).read()
    assert flags == re.search(r"^HIPFLAGS \?= (.*)$", actor_mk, re.M).group(1) and "-ffp-contract=off" in flags
    assert "UAVX_CLIP_SRC_HASH" in mk and "OUT ?= libuavx_clip.so" in mk and "SRCHASH ?=" in mk
    assert "libuavx_clip.so.tmp*" in open(os.path.join(ROOT, ".gitignore")).read().split()


def test_library_exports_exactly_what_the_header_declares():
    x = _xlib()
    hdr = open(x.HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(uavx_clip_[a-z_0-9]*)\s*\(", code))
    assert declared == set(x.SYMBOLS) == set(x.FUNCTIONS) == {"uavx_clip_version", "uavx_clip_workspace_bytes",
                                                              "uavx_clip_step"}
    assert x.SYMBOLS[0] == "uavx_clip_version"
    lib = x.load()
    for name in sorted(declared):
        assert hasattr(lib, name), name
        f = getattr(lib, name)
        assert (f.restype, list(f.argtypes)) == (x.FUNCTIONS[name][0], list(x.FUNCTIONS[name][1])), name
    assert lib.uavx_clip_version() == x.ABI_VERSION == 1 and "#define UAVX_CLIP_VERSION 1" in hdr
    for name, value in (("MAX_TENSORS", x.MAX_TENSORS), ("MAX_GROUPS", x.MAX_GROUPS), ("BLOCK", x.BLOCK)):
        assert f"#define UAVX_CLIP_{name} {value}" in hdr, name
    # the structs the binding fills have the header's fields, in its order
    for cname, cls in (("uavx_clip_record", x.Record), ("uavx_clip_group", x.Group)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.search(r"(\w+)\s*$", d).group(1) for d in body.split(";") if d.strip()]
        assert fields == [n for n, _ in cls._fields_], cname
    assert ctypes.sizeof(x.Record) == x.RECORD_BYTES == 16 and x.Record.clipped.offset == 8


def test_the_actor_library_is_untouched():
    from gym_uav_collision_avoidance_amd import _actor_lib
    assert not any("clip" in os.path.basename(f) for f in _actor_lib._sources())
    assert _actor_lib.source_hash() == "c6725b15f59f1983"
    # (a056e385b4f6651e before this library existed; moved twice since: when the weighted critic gradient became a unit, and from
    # 17c0e2c29cadcdb4 when its replay unit took the ring's view and the n-step walk from common_csrc/)


def _group(x, keep, n=12, p=None, g=None, m=None, v=None, vx=None, t=None, numel=None, lr=3e-4, b1=0.9, b2=0.999, eps=1e-8,
           tau=5e-3, step=64, scal=64):
    """A uavx_clip_group over fake addresses (64: never dereferenced); `keep` holds the ctypes arrays alive."""
    ptrs = (ctypes.c_void_p * 17)(*([64] * 17))
    num = (ctypes.c_int64 * 17)(*([8] * 17))
    keep += [ptrs, num]
    addr = lambda a: None if a is None else ctypes.addressof(a)
    pick = lambda a: ptrs if a is None else (None if a is False else a)
    return x.Group(n=n, params=addr(pick(p)), grads=addr(pick(g)), exp_avg=addr(pick(m)), exp_avg_sq=addr(pick(v)),
                   max_exp_avg_sq=addr(vx), targets=addr(t), numel=addr(num if numel is None else (None if numel is False else numel)),
                   lr=lr, beta1=b1, beta2=b2, eps=eps, tau=tau, step=step, scalars=scal)


def test_bad_arguments_refused_before_any_device_call():
    x = _xlib()
    lib = x.load()
    bad, keep = x.ERR_INVALID_ARG, []
    ptrs = (ctypes.c_void_p * 17)(*([64] * 17))
    holes = (ctypes.c_void_p * 17)(*([64] * 5 + [None] + [64] * 11))
    odd = (ctypes.c_void_p * 17)(*([64] * 5 + [66] + [64] * 11))

    def step(groups=None, count=None, work=64, work_bytes=1 << 20, max_norm=64, rec=64, **kw):
        gs = [_group(x, keep, **kw)] if groups is None else groups
        arr = (x.Group * max(1, len(gs)))(*gs)
        return lib.uavx_clip_step(len(gs) if count is None else count, arr, work, work_bytes, max_norm, rec, None)

    # every refusal below comes before a launch: the addresses are not memory
    assert step(n=0) == bad and step(n=-1) == bad and step(n=17) == bad
    assert step(p=False) == bad and step(g=False) == bad and step(m=False) == bad and step(v=False) == bad
    assert step(numel=False) == bad
    assert step(p=holes) == bad and step(g=holes) == bad and step(m=holes) == bad and step(v=holes) == bad
    assert step(vx=holes) == bad                                  # AMSGrad wants every tensor's max_exp_avg_sq
    assert step(p=odd) == bad and step(g=odd) == bad and step(t=odd) == bad and step(vx=odd) == bad     # 4-byte alignment
    for count in (0, -5, 2 ** 31):
        assert step(numel=(ctypes.c_int64 * 17)(*([8] * 3 + [count] + [8] * 13))) == bad
    assert step(step=None) == bad and step(scal=None) == bad and step(step=68) == bad and step(scal=68) == bad
    nan, inf = float("nan"), float("inf")
    for kw in (dict(lr=-1e-3), dict(lr=nan), dict(lr=inf), dict(eps=-1e-8), dict(eps=nan), dict(b1=1.0), dict(b1=-0.1),
               dict(b1=nan), dict(b2=1.0), dict(b2=-0.1), dict(b2=nan)):
        assert step(**kw) == bad, kw
    for tau in (-0.1, 1.5, nan):
        assert step(t=ptrs, tau=tau) == bad, tau
    # the call's own arguments: the device slots are 8-byte aligned, the workspace holds every block's sum
    assert step(work=None) == bad and step(max_norm=None) == bad and step(rec=None) == bad
    assert step(work=68) == bad and step(max_norm=68) == bad and step(rec=68) == bad
    assert step(work_bytes=8 * 12 - 1) == bad and step(work_bytes=0) == bad and step(work_bytes=-8) == bad
    assert step(count=0) == bad and step(count=-1) == bad and step(count=17) == bad
    assert lib.uavx_clip_step(1, None, 64, 1 << 20, 64, 64, None) == bad
    # a bad SECOND group refuses the call before the first group's launches
    good = _group(x, keep)
    assert step(groups=[good, _group(x, keep, lr=nan)]) == bad and step(groups=[good, _group(x, keep, g=holes)]) == bad
    assert step(groups=[good, good], work_bytes=8 * 24 - 1) == bad
    # the workspace: 8 bytes per 1024-element block, every tensor starting a block of its own
    need = ctypes.c_int64(-1)
    sizes = (ctypes.c_int64 * 17)(1, 1024, 1025, 2 ** 22, 2 ** 31 - 1, *([8] * 12))
    arr = (x.Group * 2)(_group(x, keep, n=5, numel=sizes), _group(x, keep, n=3))
    assert lib.uavx_clip_workspace_bytes(2, arr, ctypes.byref(need)) == x.OK
    assert need.value == 8 * (1 + 1 + 2 + 4096 + 2 ** 21 + 3)
    assert lib.uavx_clip_workspace_bytes(1, arr, ctypes.byref(need)) == x.OK and need.value == 8 * (1 + 1 + 2 + 4096 + 2 ** 21)
    assert lib.uavx_clip_workspace_bytes(0, arr, ctypes.byref(need)) == bad
    assert lib.uavx_clip_workspace_bytes(17, arr, ctypes.byref(need)) == bad
    assert lib.uavx_clip_workspace_bytes(2, None, ctypes.byref(need)) == bad
    assert lib.uavx_clip_workspace_bytes(2, arr, None) == bad
    arr = (x.Group * 1)(_group(x, keep, n=0))
    assert lib.uavx_clip_workspace_bytes(1, arr, ctypes.byref(need)) == bad


def test_kernels_use_no_scratch_and_spill_nothing():
    rows = [r for r in _kernels() if r["name"].startswith("uavx_clip_k::")]
    assert sorted(r["name"].split("::")[1] for r in rows) == ["adam_prologue", "finish", "sumsq", "update"]
    assert len(rows) == len(_kernels())                           # every kernel of the library is in the namespace
    # kernel -> (LDS bytes, VGPRs) as DESIGN.md §26 documents them: the two reductions keep four wavefront sums (32 B)
    documented = {"adam_prologue": (0, 39), "finish": (32, 39), "sumsq": (32, 12), "update": (0, 44)}
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for r in rows:
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["private_segment_fixed_size"] == 0, r
        lds, vgprs = documented[r["name"].split("::")[1]]
        assert r["group_segment_fixed_size"] == lds, r
        assert r["agpr_count"] == 0 and r["vgpr_count"] <= vgprs, r
        assert f"| `{r['name'].split('::')[1]}` | {lds} | {vgprs} |" in design, r["name"]


# ---- what the Python layer does on the host --------------------------------------------------------------------------------

def test_unclipped_fused_adam_never_imports_the_binding():
    """A fresh interpreter: importing the package, the optimiser module and the learners, and building a FusedAdam without
    max_grad_norm as far as a machine without a GPU lets it (up to the device check), leaves _clip_lib out of sys.modules;
    max_grad_norm is validated before anything else is looked at."""
    code = """
import sys, torch
sys.path.insert(0, {root!r})
import gym_uav_collision_avoidance_amd
from gym_uav_collision_avoidance_amd import fused_optim, learners
ps = [torch.nn.Parameter(torch.ones(3))]
for kw in ({{}}, dict(max_grad_norm=None)):
    try:
        fused_optim.FusedAdam(torch.optim.Adam(ps), **kw)
    except ValueError as e:
        assert "no CPU path" in str(e), e
assert not [m for m in sys.modules if m.endswith("_clip_lib")], "the binding was imported"
try:
    fused_optim.FusedAdam(torch.optim.Adam(ps), max_grad_norm=0.0)
except ValueError as e:
    assert "max_grad_norm" in str(e), e
assert not [m for m in sys.modules if m.endswith("_clip_lib")]
print("clean")
""".format(root=ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("clean"), out.stdout + out.stderr


def test_max_grad_norm_refused_on_the_host():
    from gym_uav_collision_avoidance_amd.fused_optim import FusedAdam, check_max_grad_norm
    from gym_uav_collision_avoidance_amd.learners import FusedDDPG, FusedSAC, FusedTD3
    assert check_max_grad_norm(1) == 1.0 and check_max_grad_norm(1e30) == 1e30 and check_max_grad_norm(np.float32(0.5)) == 0.5
    bad = (0, 0.0, -1.0, float("inf"), float("nan"), torch.tensor(1.0), "1", True, 1e39, 1e-50, [1.0])
    for v in bad:
        with pytest.raises(ValueError, match="uavx: max_grad_norm must be a finite float > 0"):
            check_max_grad_norm(v)
        with pytest.raises(ValueError, match="uavx: max_grad_norm must be a finite float > 0"):
            FusedAdam(torch.optim.Adam([torch.nn.Parameter(torch.ones(3))]), max_grad_norm=v)
    # the learners check the keyword before they look for a device
    for cls in (FusedSAC, FusedTD3, FusedDDPG):
        for v in bad[:-1] + ((1.0, 0.0), (None, -1.0)):
            with pytest.raises(ValueError, match=rf"uavx: {cls.__name__}: max_grad_norm must be a finite float > 0"):
                cls(device="cpu", max_grad_norm=v)
        for v in ((1.0,), (1.0, 2.0, 3.0), []):
            with pytest.raises(ValueError, match=rf"uavx: {cls.__name__}: max_grad_norm is a float or a pair"):
                cls(device="cpu", max_grad_norm=v)
        for v in (None, 1.0, (1.0, None), (None, None), [0.5, 2.0]):
            with pytest.raises(ValueError, match="uavx: the learners need a GPU"):
                cls(device="cpu", max_grad_norm=v)

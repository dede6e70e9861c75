"""Host-side checks of the weighted critic-loss gradient (a unit of libuavx_actor.so, include/uavx_wcritic_grad.h, DESIGN.md
§24): its header and every file it includes are under the actor library's source hash; the library exports exactly what the
header declares; it refuses every bad argument before touching a device; its workspace is §14's; the weighted row kernels
use no scratch and spill nothing, with the resources §24 documents; no library of its own is left and the priority library
is untouched; the learners refuse a bad per_beta on the host; and the float64 reference the GPU tests trust (wgrad_ref.py) is
grad_ref's autograd when every weight is 1."""
import ctypes
import importlib.util
import os
import re
import subprocess

import pytest
import torch

import grad_ref
import wgrad_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 64                            # a pointer that is never dereferenced: every call it goes to fails its argument check


def _xlib():
    from gym_uav_collision_avoidance_amd import _actor_lib
    _actor_lib.build()
    return _actor_lib


def _kernels():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr.kernel_table(_xlib().LIB_PATH)


# ---- the library ----------------------------------------------------------------------------------------------------------

def test_the_unit_is_under_the_actor_librarys_source_hash():
    x = _xlib()
    assert os.path.basename(x.LIB_PATH) == "libuavx_actor.so" and os.path.isfile(x.LIB_PATH)
    assert x.WGRAD_HEADER == os.path.join(ROOT, "include", "uavx_wcritic_grad.h") and x.WGRAD_HEADER in x._sources()
    names = [os.path.relpath(f, ROOT) for f in x._sources()]
    pkg = "gym_uav_collision_avoidance_amd"
    for f in (f"{pkg}/actor_csrc/uavx_critic_grad.hip", f"{pkg}/actor_csrc/uavx_grad_common.hip",
              f"{pkg}/actor_csrc/uavx_grad_impl.hpp", f"{pkg}/actor_csrc/uavx_actor_impl.hpp", "include/uavx_actor.h",
              "include/uavx_critic.h", "include/uavx_critic_grad.h"):
        assert f in names, f
    # every file the unit's translation unit includes, and every file those include, is under the hash
    unit = os.path.join(x.CSRC, "uavx_critic_grad.hip")
    assert '#include "../../include/uavx_wcritic_grad.h"' in open(unit).read()
    seen, todo = set(), [unit]
    while todo:
        f = todo.pop()
        for inc in re.findall(r'#include "([^"]+)"', open(f).read()):
            inc = os.path.normpath(os.path.join(os.path.dirname(f), inc))
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    assert seen and seen <= {os.path.normpath(f) for f in x._sources()}, seen
    blob = open(x.LIB_PATH, "rb").read()
    assert f"UAVX_ACTOR_SRC_HASH={x.source_hash()}".encode() + b"\0" in blob and b"gfx950" in blob
    assert x._up_to_date()
    mk = open(os.path.join(x.CSRC, "Makefile")).read()
    assert "../../include/uavx_wcritic_grad.h" in re.search(r"^HDR := (.*)$", mk, re.M).group(1).split()


def test_library_exports_exactly_what_the_header_declares():
    x = _xlib()
    hdr = open(x.WGRAD_HEADER).read()
    declared = set(re.findall(r"\b(uavx_wcritic_grad[a-z_0-9]*)\s*\(", hdr))
    assert declared == set(x.WGRAD_SYMBOLS) == {"uavx_wcritic_grad_version", "uavx_wcritic_grad_workspace_bytes",
                                          "uavx_wcritic_grad"}
    assert x.WGRAD_SYMBOLS[0] == "uavx_wcritic_grad_version" == x.UNITS[-1].version
    assert x.UNITS[-1].word == "weighted critic-gradient" and x.UNITS[-1].functions.keys() == declared
    lib = x.load()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.uavx_wcritic_grad_version() == x.WGRAD_ABI_VERSION == 1 and "#define UAVX_WCRITIC_GRAD_VERSION 1" in hdr
    assert f"#define UAVX_WCRITIC_GRAD_MAX_ROWS {x.GRAD_MAX_ROWS}" in hdr and x.GRAD_MAX_ROWS == 262144
    # the C symbols of the ABI's name space that the dynamic table defines are those three: nothing else of it leaks out
    out = subprocess.run(["nm", "-D", "--defined-only", x.LIB_PATH], capture_output=True, text=True, check=True).stdout
    c_names = {l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("uavx_wcritic")}
    assert c_names == declared, c_names
    # the header's numbers are the ones the binding and the other headers use
    for name, value in (("UAVX_WCRITIC_SAC", x.SAC), ("UAVX_WCRITIC_TD3", x.TD3), ("UAVX_WCRITIC_DDPG", x.DDPG),
                        ("UAVX_WCRITIC_MSE", x.GRAD_MSE), ("UAVX_WCRITIC_L1", x.GRAD_L1)):
        assert f"{name} = {value}" in hdr, name
    for name, value in (("OK", x.OK), ("ERR_INVALID_ARG", x.ERR_INVALID_ARG), ("ERR_HIP", x.ERR_HIP),
                        ("ERR_UNSUPPORTED", x.ERR_UNSUPPORTED)):
        assert re.search(r"#define UAVX_WCRITIC_%s \(?%d\)?\n" % (name, value), hdr), name


def test_no_library_of_its_own_is_left_and_the_priority_library_is_untouched():
    import gym_uav_collision_avoidance_amd as pkg
    from gym_uav_collision_avoidance_amd import _actor_lib, _prio_lib
    # 3e2046d3591a64b0 at the commit before the weighted gradient existed and until the library took the ring's view and the entry
    # plumbing from common_csrc/: the weighted gradient never touched it
    assert _prio_lib.source_hash() == "75c3f7d1033d0f00"
    assert len(_actor_lib.UNITS) == 11
    assert not any("wcritic" in os.path.basename(f) or "wgrad" in os.path.basename(f) for f in _prio_lib._sources())
    here = os.path.dirname(pkg.__file__)
    assert not os.path.exists(os.path.join(here, "wgrad_csrc")) and not os.path.exists(os.path.join(here, "_wgrad_lib.py"))
    assert importlib.util.find_spec("gym_uav_collision_avoidance_amd._wgrad_lib") is None
    assert "wgrad" not in open(os.path.join(ROOT, ".gitignore")).read()


def _call(lib, kind=0, h1=256, h2=256, towers=2, loss=0, params=True, state=P, rows=4, ss=10, action=P, as_=2, y=P, ys=1,
          weight=P, wstride=1, grads=True, loss_out=P, q_out=P, ws=P, ws_bytes=1 << 40):
    ptrs = (ctypes.c_void_p * 12)(*([P] * 12))
    return lib.uavx_wcritic_grad(kind, h1, h2, towers, loss, ptrs if params is True else params, state, rows, ss, action,
                                 as_, y, ys, weight, wstride, ptrs if grads is True else grads, loss_out, q_out, ws, ws_bytes,
                                 None)


def test_bad_arguments_refused_before_any_device_call():
    x = _xlib()
    lib = x.load()
    bad, uns = x.ERR_INVALID_ARG, x.ERR_UNSUPPORTED
    n = ctypes.c_int64(7)
    need = ctypes.c_int64()
    assert lib.uavx_wcritic_grad_workspace_bytes(x.SAC, 256, 256, 2, 4, ctypes.byref(need)) == x.OK and need.value > 0
    # null pointers
    for name in ("state", "action", "y", "loss_out", "ws"):
        assert _call(lib, **{name: None}) == bad, name
    assert _call(lib, params=None) == bad and _call(lib, grads=None) == bad
    holes = (ctypes.c_void_p * 12)(*([P] * 12))
    holes[7] = None
    assert _call(lib, params=holes) == bad and _call(lib, grads=holes) == bad
    assert lib.uavx_wcritic_grad_workspace_bytes(x.SAC, 256, 256, 2, 256, None) == bad
    # rows
    for rows in (0, -3, 262145, 2 ** 40):
        assert _call(lib, rows=rows) == bad, rows
        assert lib.uavx_wcritic_grad_workspace_bytes(x.SAC, 256, 256, 2, rows, ctypes.byref(n)) == bad and n.value == 0
    # widths: check_handle's limits, 241..256 for the twins and 385..400 for DDPG
    for kind, towers, h1s in ((x.SAC, 2, (240, 257, 384, 401, 0, -1)), (x.TD3, 2, (240, 257, 384, 401)),
                              (x.DDPG, 1, (240, 257, 384, 401, 256))):
        for h1 in h1s:
            assert _call(lib, kind=kind, towers=towers, h1=h1) in (bad, uns), (kind, h1)
            assert lib.uavx_wcritic_grad_workspace_bytes(kind, h1, 256, towers, 256, ctypes.byref(n)) in (bad, uns)
            assert n.value == 0
    for kind, towers, h1s in ((x.SAC, 2, (241, 256)), (x.TD3, 2, (241, 256)), (x.DDPG, 1, (385, 400))):
        for h1 in h1s:
            assert lib.uavx_wcritic_grad_workspace_bytes(kind, h1, 17, towers, 256, ctypes.byref(n)) == x.OK, (kind, h1)
    for h2 in (0, -1):
        assert _call(lib, h2=h2) == bad
    for towers in (0, 3, -1):
        assert _call(lib, towers=towers) == bad, towers
    for kind in (-1, 3):
        assert _call(lib, kind=kind) == bad, kind
    for loss in (2, -1):
        assert _call(lib, loss=loss) == bad, loss
    # strides
    assert _call(lib, ss=9) == bad and _call(lib, ss=-10) == bad and _call(lib, as_=1) == bad and _call(lib, as_=-2) == bad
    assert _call(lib, ys=0) == bad and _call(lib, ys=-1) == bad
    assert _call(lib, wstride=0) == bad and _call(lib, wstride=-1) == bad
    # the workspace: misaligned, short
    assert _call(lib, ws=P + 4) == bad and _call(lib, ws=P + 8) == bad
    assert _call(lib, ws_bytes=need.value - 1) == bad and _call(lib, ws_bytes=0) == bad


def _section14_bytes(h1, h2, T, rows):
    """DESIGN.md §14's workspace, written out."""
    def align(v):
        return (v + 255) // 256 * 256
    b16 = (rows + 15) // 16 * 16
    n1, n2 = 16 * -(-h1 // 16), 16 * -(-h2 // 16)
    lp = (13 * h1 + 2 * h2 + 2 + 3) // 4 * 4
    tiles = T * -(-h2 // 64) * -(-h1 // 64)
    S = min(-(-b16 // 64), max(1, 8192 // tiles))
    kc = 16 * -(-(-(-b16 // S)) // 16)
    S = -(-b16 // kc)
    return (align(T * b16 * n1 * 4) + align(T * b16 * n2 * 4) + align(T * (b16 // 16) * lp * 8)
            + align(S * T * h2 * h1 * 4) + align(S * T * lp * 8)), S


def test_workspace_bytes_are_section_14s():
    x = _xlib()
    lib = x.load()
    n = ctypes.c_int64()
    for kind, h1, h2, T, rows, slices in ((x.SAC, 256, 256, 2, 256, 4), (x.DDPG, 400, 300, 1, 17, 1)):
        want, S = _section14_bytes(h1, h2, T, rows)
        assert S == slices
        assert lib.uavx_wcritic_grad_workspace_bytes(kind, h1, h2, T, rows, ctypes.byref(n)) == x.OK
        assert n.value == want, (kind, n.value, want)


def test_kernels_use_no_scratch_and_spill_nothing():
    unit = ("uavx_critic_grad_k::grad_combine", "uavx_critic_grad_k::grad_rows<false, 16, true>",
            "uavx_critic_grad_k::grad_rows<true, 25, true>", "uavx_grad_k::grad_weights")
    rows = [r for r in _kernels() if r["name"] in unit]
    assert sorted(r["name"] for r in rows) == sorted(unit)
    # kernel -> (LDS bytes, VGPRs, AGPRs) as DESIGN.md §24 documents them: the weighted row pass keeps the unweighted one's
    # budget (one workgroup per CU: 216 registers for the twins, 360 + 136 for DDPG); the other two launches are shared
    documented = {"grad_rows<false, 16, true>": (83584, 216, 64), "grad_rows<true, 25, true>": (129664, 360, 136),
                  "grad_weights": (0, 92, 64), "grad_combine": (0, 14, 0)}
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for r in rows:
        short = r["name"].split("::")[1]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["private_segment_fixed_size"] == 0, r
        assert r["max_flat_workgroup_size"] == 256, r
        lds, vgprs, agprs = documented[short]
        assert r["group_segment_fixed_size"] == lds, r
        assert r["vgpr_count"] <= vgprs and r["agpr_count"] <= agprs, r
        assert f"| `{short}` | {lds} | {vgprs} | {agprs} |" in design, short


# ---- what the Python layer refuses on the host -----------------------------------------------------------------------------

def test_learners_refuse_a_bad_per_beta_before_the_device():
    from gym_uav_collision_avoidance_amd.learners import FusedDDPG, FusedSAC, FusedTD3
    for cls in (FusedSAC, FusedTD3, FusedDDPG):
        for beta in (-0.1, 1.5, float("nan"), float("inf"), "x", None):
            with pytest.raises(ValueError, match=rf"uavx: {cls.__name__} takes an importance-sampling exponent per_beta in "
                                                 r"\[0, 1\]"):
                cls(device="cpu", prioritized=0.6, per_beta=beta)
        with pytest.raises(ValueError, match="per_beta=0.4 needs prioritized=alpha"):
            cls(device="cpu", per_beta=0.4)
        with pytest.raises(ValueError, match="per_beta=1 needs prioritized=alpha"):
            cls(device="cpu", per_beta=1, prioritized=None)
        # good values get as far as the device
        for kw in (dict(prioritized=0.6, per_beta=0.4), dict(prioritized=0.6, per_beta=0.0), dict(per_beta=0.0),
                   dict(prioritized=0.6, per_beta=1)):
            with pytest.raises(ValueError, match="uavx: the learners need a GPU"):
                cls(device="cpu", **kw)


# ---- the reference ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["mse", "l1"])
@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_weighted_reference_with_unit_weights_is_grad_ref(kind, loss):
    m = grad_ref.critic(kind, 3, hidden1=24 if kind != "ddpg" else 40, hidden2=17).double()
    g = torch.Generator().manual_seed(1)
    B = 37
    s = torch.randn((B, 10), generator=g, dtype=torch.float64)
    a = torch.rand((B, 2), generator=g, dtype=torch.float64) * 2 - 1
    y = torch.randn((B,), generator=g, dtype=torch.float64)
    gw, lw, qw = wgrad_ref.autograd(m, s, a, y, torch.ones(B, dtype=torch.float64), loss)
    gr, lr = grad_ref.autograd(m, s, a, y, loss)
    assert len(gw) == len(gr) == (6 if kind == "ddpg" else 12) and len(qw) == len(lw) == len(lr)
    for x, r in zip(gw + lw, gr + lr):
        assert x.shape == r.shape and torch.allclose(x, r, rtol=1e-13, atol=1e-15), float((x - r).abs().max())
    out = m(s, a)
    for q, r in zip(qw, out if isinstance(out, tuple) else (out,)):
        assert torch.equal(q, r.detach().reshape(-1))
    # a weight matters, and enters linearly: w = 2 doubles everything, a random w does not
    g2, l2, _ = wgrad_ref.autograd(m, s, a, y, torch.full((B, 1), 2.0, dtype=torch.float64), loss)
    for x, r in zip(g2 + l2, gr + lr):
        assert torch.allclose(x, 2 * r, rtol=1e-13, atol=1e-15)
    w = torch.rand(B, generator=g, dtype=torch.float64)
    g3, _, _ = wgrad_ref.autograd(m, s, a, y, w, loss)
    assert max(float((x - r).abs().max()) for x, r in zip(g3, gr)) > 1e-6

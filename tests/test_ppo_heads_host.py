"""Host-side checks of PPO's HIP heads (libuavx_ppo.so, include/uavx_ppo.h): the analytic gradients of the
restatement the GPU tests trust (ppo_heads_ref.py) equal autograd's on the float64 loss written with torch's own minimum and
clamp, its log density equals ppo_ref's, the library builds for gfx950 without a GPU, carries its source hash, exports exactly
what its header declares and refuses every bad argument before touching a device; the other libraries keep their pinned
hashes; the Python layers refuse bad arguments on the host and a default PPO never loads the library."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import gae_layouts
import ppo_heads_ref
import ppo_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP, VF, ENT = 0.2, 0.5, 0.01


def _xlib():
    from gym_uav_collision_avoidance_amd import _ppo_lib
    _ppo_lib.build()
    return _ppo_lib


# ---- the restatement -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("identity", [False, True], ids=["idx", "identity"])
def test_analytic_gradients_equal_autograd_on_the_float64_loss(identity):
    c = ppo_heads_ref.make_case(1000, seed=3, identity=identity)
    ref = ppo_heads_ref.loss(clip=CLIP, vf_coef=VF, ent_coef=ENT, dtype=torch.float64, **c)
    live = ref["w"] > 0
    for sign in (ref["adv"] > 0, ref["adv"] < 0):
        for side in (ref["ratio"] < 1 - CLIP, ref["ratio"] > 1 + CLIP, (ref["ratio"] > 1 - CLIP) & (ref["ratio"] < 1 + CLIP)):
            assert int((live & sign & side).sum()) >= 30
    mean, log_std, v = (c[k].double().requires_grad_() for k in ("mean", "log_std", "v"))
    idx = torch.arange(1000) if identity else c["idx"]
    u, logp_old, adv, ret, w = (c[k].double()[idx] for k in ("u", "logp_old", "adv", "ret", "weight"))
    logp, _ = ppo_ref.log_density(mean, log_std, u)
    ratio = torch.exp(logp - logp_old)
    surrogate = torch.minimum(ratio * adv, ratio.clamp(1 - CLIP, 1 + CLIP) * adv)
    denom = w.sum().clamp(min=1.0)
    policy_loss, value_loss = -(w * surrogate).sum() / denom, (w * (0.5 * (v - ret) ** 2)).sum() / denom
    entropy = -(w * logp).sum() / denom
    (policy_loss + VF * value_loss - ENT * entropy).backward()
    for name, got, want in (("g_mean", ref["g_mean"], mean.grad), ("g_log_std", ref["g_log_std"], log_std.grad),
                            ("g_v", ref["g_v"], v.grad), ("ratio", ref["ratio"], ratio.detach()),
                            ("policy_loss", ref["policy_loss"], policy_loss.detach()),
                            ("value_loss", ref["value_loss"], value_loss.detach()), ("entropy", ref["entropy"], entropy.detach())):
        d = ppo_ref.distance(got, want)
        print(f"{name:12s} distance from autograd {d:.3e}")
        assert d <= 1e-12, name
    assert float(ref["n"]) == float(w.sum()) and 0.6 * 1000 < float(ref["n"]) < 0.9 * 1000


def test_log_density_equals_ppo_ref():
    """Two writings of log(1 − tanh²u) -- 2·(log 2 − u − softplus(−2u)) here, log 4 − 2|u| − 2·log1p(exp(−2|u|)) there -- in
    float64, out to |u| = 20 and log σ = −20: a few float64 roundings of Σ|terms| apart."""
    c = ppo_heads_ref.make_case(1000, seed=4)
    u = c["u"][c["idx"]].double()
    assert float(u.abs().max()) == 20.0 and float(c["log_std"].min()) == -20.0 and float(c["log_std"].max()) == 2.0
    got, _ = ppo_heads_ref.log_density(c["mean"].double(), c["log_std"].double(), u)
    want, scale = ppo_ref.log_density(c["mean"].double(), c["log_std"].double(), u)
    assert bool(((got - want).abs() <= 2.0 ** -48 * scale).all())


def test_sample_restatement_is_the_density_of_its_own_sample():
    g = torch.Generator().manual_seed(6)
    mean, log_std, eps = torch.randn((50, 2), generator=g), torch.rand((50, 2), generator=g) - 1, torch.randn((50, 2), generator=g)
    u, a, logp = ppo_heads_ref.sample(mean, log_std, eps, torch.float64)
    assert torch.equal(a, torch.tanh(u)) and torch.equal(u, mean.double() + torch.exp(log_std.double()) * eps.double())
    want, scale = ppo_ref.log_density(mean.double(), log_std.double(), u)
    assert bool(((logp - want).abs() <= 2.0 ** -48 * scale).all())


# ---- the library -----------------------------------------------------------------------------------------------------------

def test_library_cross_compiles_and_carries_its_source_hash():
    x = _xlib()
    assert os.path.basename(x.LIB_PATH) == "libuavx_ppo.so" and os.path.isfile(x.LIB_PATH)
    assert x.HEADER == os.path.join(ROOT, "include", "uavx_ppo.h") and x.HEADER in x._sources()
    assert any(f.endswith(os.path.join("ppo_csrc", "uavx_ppo.hip")) for f in x._sources())
    blob = open(x.LIB_PATH, "rb").read()
    assert f"UAVX_PPO_SRC_HASH={x.source_hash()}".encode() + b"\0" in blob and b"gfx950" in blob
    assert x._up_to_date()
    mk = open(os.path.join(x.CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, re.M).group(1)
    gae_mk = open(os.path.join(ROOT, "gym_uav_collision_avoidance_amd", "gae_csrc", "Makefile")).read()
    assert flags == re.search(r"^HIPFLAGS \?= (.*)$", gae_mk, re.M).group(1) and "-ffp-contract=off" in flags
    assert "UAVX_PPO_SRC_HASH" in mk and "OUT ?= libuavx_ppo.so" in mk and "SRCHASH ?=" in mk
    assert "libuavx_ppo.so.tmp*" in open(os.path.join(ROOT, ".gitignore")).read().split()


def test_library_exports_exactly_what_the_header_declares():
    x = _xlib()
    hdr = open(x.HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(uavx_ppo_[a-z_0-9]*)\s*\(", code))
    assert declared == set(x.SYMBOLS) == set(x.FUNCTIONS) == {"uavx_ppo_version", "uavx_ppo_sample",
                                                              "uavx_ppo_loss_workspace_bytes", "uavx_ppo_loss"}
    assert x.SYMBOLS[0] == "uavx_ppo_version"
    lib = x.load()
    for name in sorted(declared):
        f = getattr(lib, name)
        assert (f.restype, list(f.argtypes)) == (x.FUNCTIONS[name][0], list(x.FUNCTIONS[name][1])), name
    assert lib.uavx_ppo_version() == x.ABI_VERSION == 1 and "#define UAVX_PPO_VERSION 1" in hdr
    assert f"#define UAVX_PPO_BLOCK {x.BLOCK}" in hdr and x.BLOCK == 256
    nm = subprocess.run(["nm", "-D", "--defined-only", x.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l and "uavx" in l and not l.split()[-1].startswith("_Z")}
    assert exported == declared


def test_bad_arguments_refused_before_any_device_call():
    x = _xlib()
    lib = x.load()
    bad, nan, inf = x.ERR_INVALID_ARG, float("nan"), float("inf")

    # every refusal below comes before a launch: the addresses are not memory
    def sample(mean=64, log_std=64, eps=64, rows=100, u=64, logp=64, action=64):
        return lib.uavx_ppo_sample(mean, log_std, eps, rows, u, logp, action, None)

    for name in ("mean", "log_std", "eps", "u", "logp", "action"):
        assert sample(**{name: None}) == bad, name
    for name in ("mean", "log_std", "eps", "u", "action"):
        assert sample(**{name: 68}) == bad, name                            # [rows, 2] arrays are read as 8-byte pairs
    assert sample(logp=66) == bad
    assert sample(rows=0) == bad and sample(rows=-1) == bad and sample(rows=2 ** 31) == bad

    def loss(mean=64, log_std=64, v=64, idx=64, B=100, u=64, logp_old=64, adv=64, ret=64, weight=64, R=203, clip=0.2, vf=0.5,
             ent=0.0, ratio=64, scalars=64, g_mean=64, g_log_std=64, g_v=64, work=64, work_bytes=1 << 20):
        return lib.uavx_ppo_loss(mean, log_std, v, idx, B, u, logp_old, adv, ret, weight, R, clip, vf, ent, ratio, scalars,
                                 g_mean, g_log_std, g_v, work, work_bytes, None)

    pointers = ("mean", "log_std", "v", "u", "logp_old", "adv", "ret", "weight", "ratio", "scalars", "g_mean", "g_log_std",
                "g_v", "work")
    for name in pointers:
        assert loss(**{name: None}) == bad, name
    for name in ("mean", "log_std", "u", "g_mean", "g_log_std", "idx", "work"):
        assert loss(**{name: 68}) == bad, name
    for name in ("v", "logp_old", "adv", "ret", "weight", "ratio", "scalars", "g_v"):
        assert loss(**{name: 66}) == bad, name
    assert loss(B=0) == bad and loss(B=-5) == bad and loss(B=2 ** 31) == bad
    assert loss(R=0) == bad and loss(R=-1) == bad and loss(R=2 ** 31) == bad
    assert loss(idx=None, B=100, R=99) == bad                                # the identity needs B <= R
    for c in (0.0, -0.2, nan, inf, -inf):
        assert loss(clip=c) == bad, c
    for c in (-1e-9, -1.0, nan, inf, -inf):
        assert loss(vf=c) == bad and loss(ent=c) == bad, c
    assert loss(work_bytes=31) == bad and loss(work_bytes=0) == bad and loss(work_bytes=-32) == bad
    assert loss(B=257, R=600, work_bytes=63) == bad                          # two workgroups
    need = ctypes.c_int64(-1)
    for B, want in ((1, 32), (256, 32), (257, 64), (65537, 32 * 257), (2 ** 31 - 1, 32 * 2 ** 23)):
        assert lib.uavx_ppo_loss_workspace_bytes(B, ctypes.byref(need)) == x.OK and need.value == want, B
    assert lib.uavx_ppo_loss_workspace_bytes(100, None) == bad
    for B in (0, -1, 2 ** 31):
        assert lib.uavx_ppo_loss_workspace_bytes(B, ctypes.byref(need)) == bad


def test_the_other_libraries_keep_their_hashes():
    from gym_uav_collision_avoidance_amd import _actor_lib, _gae_lib, _lib, _prio_lib
    assert _actor_lib.source_hash() == "c6725b15f59f1983"        # 17c0e2c29cadcdb4 before its replay unit took the ring's view and the n-step walk from common_csrc/
    assert _prio_lib.source_hash() == "75c3f7d1033d0f00"         # 3e2046d3591a64b0 before it took the ring's view and the entry plumbing from common_csrc/
    assert _lib.source_hash() == "c85b3516db0d8e1b"
    for mod in (_actor_lib, _prio_lib, _lib, _gae_lib):
        assert not any("ppo" in os.path.basename(f) for f in mod._sources())


# ---- what the Python layers do on the host -----------------------------------------------------------------------------------

def test_heads_arguments_refused_on_the_host():
    from gym_uav_collision_avoidance_amd import _ppo_lib
    from gym_uav_collision_avoidance_amd.ppo_heads import PPOHeads
    was = _ppo_lib.loaded()
    heads = PPOHeads("cpu")
    c = ppo_heads_ref.make_case(10, seed=1)
    args = dict(c, clip=0.2, vf_coef=0.5, ent_coef=0.0)
    z2, z1 = torch.zeros((10, 2)), torch.zeros(10)
    for name, wrong in (("mean", c["mean"].double()), ("mean", c["mean"][:9]), ("log_std", c["log_std"].t().contiguous().t()),
                        ("v", c["v"].double()), ("v", c["v"].numpy()), ("v", torch.zeros((10, 1))), ("idx", c["idx"].int()),
                        ("idx", c["idx"][:9]), ("u", c["u"][:, :1]), ("u", c["u"][:-1]), ("logp_old", c["logp_old"][1:]),
                        ("adv", c["adv"].half()), ("ret", None), ("weight", c["weight"].bool()), ("weight", None),
                        ("mean", c["mean"].to("meta"))):
        with pytest.raises(ValueError, match="uavx: PPOHeads: "):
            heads.loss(**dict(args, **{name: wrong}))
    for name, wrong in (("clip", 0.0), ("clip", float("nan")), ("clip", True), ("clip", "0.2"), ("vf_coef", -0.1),
                        ("ent_coef", float("inf")), ("ent_coef", None)):
        with pytest.raises(ValueError, match=f"PPOHeads: {name} must be a finite float"):
            heads.loss(**dict(args, **{name: wrong}))
    with pytest.raises(ValueError, match="without idx"):
        heads.loss(**dict(args, idx=None, u=c["u"][:9], logp_old=c["logp_old"][:9], adv=c["adv"][:9], ret=c["ret"][:9],
                          weight=c["weight"][:9]))
    sample = dict(mean=z2, log_std=z2, eps=z2, u_out=z2.clone(), logp_out=z1.clone(), action_out=z2.clone())
    for name, wrong in (("mean", z1), ("mean", z2.double()), ("log_std", z2[:5]), ("eps", z2.t().contiguous().t()),
                        ("u_out", z2[::2]), ("logp_out", z2), ("action_out", None), ("mean", torch.zeros((0, 2)))):
        with pytest.raises(ValueError, match="uavx: PPOHeads: "):
            heads.sample(**dict(sample, **{name: wrong}))
    for rows in (0, -1, 2 ** 31, 1.5, True):
        with pytest.raises(ValueError, match="rows must be an int"):
            heads.reserve(rows)
    # everything fits: what is left is that there is no CPU path
    for call in (lambda: heads.loss(**args), lambda: heads.sample(**sample), lambda: heads.reserve(10)):
        with pytest.raises(ValueError, match="no CPU path"):
            call()
    assert _ppo_lib.loaded() == was                                          # none of this needed the library


def test_fused_heads_must_be_a_bool_and_the_default_learner_never_loads_the_library():
    import sys
    from gym_uav_collision_avoidance_amd.ppo import PPO
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r); import gae_layouts\n"
            "from gym_uav_collision_avoidance_amd.ppo import PPO\n"
            "mem = gae_layouts.CraftedRing(gae_layouts.make('count_9', 4, 2), 'cpu')\n"
            "ppo = PPO(mem, generator=torch.Generator().manual_seed(1)); ppo.act()\n"
            "assert ppo.fused_heads is False and ppo.heads is None\n"
            "mods = [m for m in sys.modules if m.endswith('._ppo_lib') or m.endswith('.ppo_heads')]\n"
            "assert not mods, mods\n"
            "from gym_uav_collision_avoidance_amd import _ppo_lib\n"
            "assert not _ppo_lib.loaded()\n"
            "fused = PPO(mem, fused_heads=True)\n"
            "assert fused.fused_heads is True and 'fused_heads' not in fused.state_dict() and not _ppo_lib.loaded()\n"
            "print('ok')\n") % (ROOT, os.path.join(ROOT, "tests"))
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stderr
    mem = gae_layouts.CraftedRing(gae_layouts.make("count_9", 4, 2), "cpu")
    for wrong in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="fused_heads must be a bool"):
            PPO(mem, fused_heads=wrong)
    fused = PPO(mem, fused_heads=True)
    with pytest.raises(ValueError, match="no CPU path"):
        fused.act()

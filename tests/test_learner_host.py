"""Host-side checks of the learners (gym_uav_collision_avoidance_amd/learners.py, include/uavx_learner.h): the float32
restatement (tests/learner_ref.py) meets the project's distance rule against the fixture's float64 samples and returns the
reference's scalars, the float64 restatement reproduces the fixture, the header declares what _actor_lib binds, the library
cross-compiles with the new unit under the source hash and exports it, the tail rejects bad arguments before touching a
device, its kernel uses no scratch, and the alpha-step formula the GPU tests trust equals torch.optim.Adam in float64."""
import ctypes
import importlib.util
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import learner_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _alib():
    from gym_uav_collision_avoidance_amd import _actor_lib
    _actor_lib.build()
    return _actor_lib


@pytest.fixture(scope="module", params=lr.KINDS)
def case(request):
    return request.param, lr.load_fixture(request.param, GOLDEN)


def test_fixture_holds_only_the_documented_arrays(case):
    kind, fx = case
    names = list(lr.sample_indices(kind))
    want = {f"idx_{n}" for n in names}
    for rows in lr.CASES:
        p = f"b{rows}_"
        want |= {p + k for k in ("state", "action", "reward", "next_state", "mask", "noise", "scalars_ref", "scalars_f64",
                                 "scalars_f32")}
        want |= {p + d + n for d in ("f32_", "f64_") for n in names}
        assert fx[p + "state"].shape == (lr.K, rows, 10) and fx[p + "noise"].shape[2:] == (rows, 2)
    assert set(fx) == want
    with np.load(os.path.join(GOLDEN, f"learner_updates_{kind}.npz")) as z:
        meta = json.loads(str(z["meta"]))
    assert meta["kind"] == "learner_updates" and meta["learner"] == kind and meta["rows"] == list(lr.CASES)
    for n, idx in lr.sample_indices(kind).items():
        assert np.array_equal(fx["idx_" + n], idx)
    assert os.path.getsize(os.path.join(GOLDEN, f"learner_updates_{kind}.npz")) < 512 * 1024


@pytest.mark.parametrize("rows", lr.CASES)
def test_float32_restatement_meets_the_rule_and_returns_the_reference_scalars(case, rows):
    kind, fx = case
    batches, noises = lr.case_inputs(fx, rows)
    agent, scalars = lr.run(kind, batches, noises, torch.float32)
    idx = {n[4:]: fx[n] for n in fx if n.startswith("idx_")}
    lr.check_networks(lr.sampled(agent.tensors(), idx), fx, rows, f"{kind} float32 restatement")
    ref = fx[f"b{rows}_scalars_ref"]
    if kind == "td3":
        assert np.isnan(ref).all()                       # td3.py's update_parameters returns None
        return
    assert not np.isnan(ref).any()
    err = np.abs(scalars - ref)
    print(kind, rows, "largest relative difference of a returned scalar", float((err / np.maximum(np.abs(ref), 1e-30)).max()))
    assert (err <= 1e-6 * np.abs(ref)).all(), err
    if kind == "sac":
        # update 0: log_alpha is 0, so alpha_loss is a zero; the returned alpha is already exp(log_alpha) after the step,
        # while the losses of that update were formed with alpha = 2 (the restatement started at 1 is far away)
        assert ref[0, 3] == 0.0 and scalars[0, 3] == 0.0
        assert np.signbit(ref[0, 3]) == np.signbit(scalars[0, 3])
        assert np.float32(ref[0, 4]) == np.float32(scalars[0, 4]) and abs(ref[0, 4] - math.exp(-3e-4)) < 1e-6
        _, one = lr.run(kind, batches[:1], noises[:1], torch.float32, alpha0=1.0)
        assert abs(one[0, 2] - ref[0, 2]) > 1e-2 * abs(ref[0, 2])


@pytest.mark.parametrize("rows", lr.CASES)
def test_float64_restatement_reproduces_the_fixture(case, rows):
    kind, fx = case
    batches, noises = lr.case_inputs(fx, rows)
    agent, scalars = lr.run(kind, batches, noises, torch.float64)
    idx = {n[4:]: fx[n] for n in fx if n.startswith("idx_")}
    for n, v in lr.sampled(agent.tensors(), idx).items():
        ref = fx[f"b{rows}_f64_{n}"]
        assert np.abs(v - ref).max() <= 1e-12, n
    assert np.abs(scalars - fx[f"b{rows}_scalars_f64"]).max() <= 1e-12


def test_learner_exports_every_declared_symbol():
    a = _alib()
    hdr = open(a.LEARNER_HEADER).read()
    declared = set(re.findall(r"\b(uavx_learner[a-z_0-9]*)\s*\(", hdr))
    assert declared == set(a.LEARNER_SYMBOLS), declared ^ set(a.LEARNER_SYMBOLS)
    assert set(a.LEARNER_SYMBOLS).isdisjoint(a.SYMBOLS + a.CRITIC_SYMBOLS + a.GRAD_SYMBOLS + a.OPTIM_SYMBOLS
                                             + a.REPLAY_SYMBOLS + a.ACTION_GRAD_SYMBOLS + a.POLICY_GRAD_SYMBOLS)
    lib = a.load()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.uavx_learner_version() == a.LEARNER_ABI_VERSION == 1
    assert "#define UAVX_LEARNER_VERSION 1" in hdr
    assert f"#define UAVX_LEARNER_LOG_COLUMNS {a.LEARNER_LOG_COLUMNS}" in hdr


def test_learner_library_cross_compiles_and_hash_covers_header():
    a = _alib()
    assert a.LEARNER_HEADER in a._sources()
    assert any(f.endswith("uavx_learner.hip") for f in a._sources())
    assert f"UAVX_ACTOR_SRC_HASH={a.source_hash()}".encode() in open(a.LIB_PATH, "rb").read()
    mk = open(os.path.join(a.CSRC, "Makefile")).read()
    assert "uavx_learner.hip" in mk and "uavx_learner.h" in mk
    nm = subprocess.run(["nm", "-D", "--defined-only", a.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert set(a.LEARNER_SYMBOLS) <= exported
    assert {s for s in exported if s.startswith("uavx_learner")} == set(a.LEARNER_SYMBOLS)


def test_tail_bad_arguments_rejected_before_any_device_call():
    a = _alib()
    lib = a.load()
    buf = ctypes.c_void_p(64)      # never dereferenced: every call that gets it fails its argument check first
    three = (ctypes.c_void_p * 3)(64, 64, 64)

    def tail(kind=a.SAC, losses=three, lpm=buf, te=-2.0, la=buf, m=buf, v=buf, step=buf, lr=3e-4, b1=0.9, b2=0.999,
             eps=1e-8, alpha=buf, log=buf, cap=4, updates=buf, au=1):
        return lib.uavx_learner_tail(kind, losses, lpm, te, la, m, v, step, lr, b1, b2, eps, alpha, log, cap, updates, au,
                                     None)

    bad = a.ERR_INVALID_ARG
    assert tail(cap=0) == bad and tail(cap=-1) == bad
    assert tail(log=None) == bad
    assert tail(lr=-1e-3) == bad and tail(lr=float("nan")) == bad and tail(lr=float("inf")) == bad
    assert tail(kind=3) == bad and tail(kind=-1) == bad
    assert tail(losses=None) == bad
    assert tail(losses=(ctypes.c_void_p * 3)(None, 64, 64)) == bad
    assert tail(losses=(ctypes.c_void_p * 3)(66, 64, 64)) == bad           # not 4-byte aligned
    assert tail(updates=None) == bad and tail(updates=ctypes.c_void_p(68)) == bad
    assert tail(au=2) == bad and tail(au=-1) == bad
    assert tail(log=ctypes.c_void_p(66)) == bad
    for name in ("lpm", "m", "v", "step", "alpha"):                        # the alpha step needs all of them
        assert tail(**{name: None}) == bad, name
    assert tail(step=ctypes.c_void_p(68)) == bad
    assert tail(kind=a.TD3) == bad and tail(kind=a.DDPG) == bad            # log_alpha with a learner that has none
    assert tail(b1=1.0) == bad and tail(b2=-0.1) == bad and tail(eps=-1e-8) == bad
    assert tail(te=float("nan")) == bad and tail(te=float("inf")) == bad


def test_tail_kernel_is_one_wavefront_without_scratch():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.kernel_table(_alib().LIB_PATH)
    mine = [r for r in rows if r["name"].startswith("uavx_learner_k::")]
    assert [r["name"] for r in mine] == ["uavx_learner_k::tail"]
    r = mine[0]
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0
    assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0
    assert r["max_flat_workgroup_size"] == 64
    rec = json.load(open(os.path.join(ROOT, "profiles", "r15_learner_kernel_resources.json")))
    assert [x["name"] for x in rec] == ["uavx_learner_k::tail"]
    for f in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
              "max_flat_workgroup_size"):
        assert rec[0][f] == r[f], (f, rec[0][f], r[f])
    # the other units keep their kernels
    assert sum(x["name"].startswith("uavx_optim_k::") for x in rows) == 3
    assert sum(x["name"].startswith("uavx_policy_grad_k::") for x in rows) == 5


def test_alpha_step_formula_equals_torch_adam_in_float64():
    """§15's own check and bound: 200 steps of a one-element tensor, 1e-13."""
    rs = np.random.RandomState(5)
    hs = rs.normal(0.0, 2.0, 200)
    hs[:3] = (0.0, -3.0 + 2.0, 2.5 - 2.0)
    la_t = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([la_t], lr=3e-4)
    la = m = v = 0.0
    for t, h in enumerate(hs, start=1):
        loss_t = -(la_t * float(h)).mean()
        opt.zero_grad()
        loss_t.backward()
        opt.step()
        loss, la, m, v, alpha = lr.alpha_step(la, m, v, t, h)
        st = opt.state[la_t]
        assert abs(float(loss_t.detach()) - loss) <= 1e-13
        assert abs(float(la_t.detach()) - la) <= 1e-13
        assert abs(float(st["exp_avg"]) - m) <= 1e-13
        assert abs(float(st["exp_avg_sq"]) - v) <= 1e-13
        assert abs(float(la_t.detach().exp()) - alpha) <= 1e-13
    assert la != 0.0


def test_ddpg_networks_start_as_the_reference_initialises_them():
    """pytorch_ddpg_temp/model.py:19-22, 48-51: input and fc1 weights within +-1/sqrt(out features) (fanin_init divides by
    size[0]), fc2 within +-5e-4 (actor) / +-5e-5 (critic), each layer filling its range (the largest of >= 300 uniform draws
    is above 0.9 of the bound but for a chance of 1e-14); torch's default would put fc2 at +-1/sqrt(300) = 0.058."""
    from gym_uav_collision_avoidance_amd import learners, policy
    torch.manual_seed(11)
    for net, init_w in ((policy.DDPGActor(), 5e-4), (policy.DDPGCritic(), 5e-5)):
        before = [p.detach().clone() for p in (net.input.bias, net.fc1.bias, net.fc2.bias)]
        assert learners.ddpg_init(net, init_w) is net
        for lin, bound in ((net.input, 1 / math.sqrt(400)), (net.fc1, 1 / math.sqrt(300)), (net.fc2, init_w)):
            top = float(lin.weight.detach().abs().max())
            assert 0.9 * bound < top <= bound, (type(net).__name__, tuple(lin.weight.shape), top, bound)
            assert abs(float(lin.weight.detach().mean())) < 0.1 * bound
        for b, p in zip(before, (net.input.bias, net.fc1.bias, net.fc2.bias)):
            assert torch.equal(b, p)                     # the reference leaves the biases at nn.Linear's default


def test_python_learners_refuse_a_cpu_before_the_device():
    from gym_uav_collision_avoidance_amd import learners
    for cls in (learners.FusedSAC, learners.FusedTD3, learners.FusedDDPG):
        with pytest.raises(ValueError, match="no CPU path"):
            cls(device="cpu")

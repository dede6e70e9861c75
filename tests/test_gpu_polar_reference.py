"""GPU tests of polar="reference" (UAVX_ACTION_POLAR_REFERENCE): the trainers' polar conversion with their own dtypes on every
step_ex kernel path.  Checked against the committed recording of the reference trainer loop (tests/golden/trainer_loop_*.npz,
value for value), against the oracle's cartesian step fed the host restatement's commands (independent of the new device
code), and through the public surfaces.  The float64 (warm-up) branch's commands may differ from glibc's by an ulp; the rate
is measured by test_conversion_kernel_* and the bound used below is the one DESIGN.md section 12 states."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

from golden_util import obs_err, tie_agents
from test_polar_reference_host import edge_actions, restate, same_bits

pytestmark = pytest.mark.gpu
TOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
VEL64_RTOL = 1e-12     # after a float64-action step: the command may be an ulp or two off glibc's


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available()
    import gym_uav_collision_avoidance_amd as pkg
    return pkg


def _np(t):
    return t.detach().cpu().numpy()


def _fixture(kind):
    d = np.load(os.path.join(GOLDEN, f"trainer_loop_{kind}.npz"))
    return {k: d[k] for k in d.files}, json.loads(str(d["meta"]))


def _groups(d):
    """Episodes that can share one batch: all-float64 actions, all-float32 actions, and each mixed episode on its own."""
    ep, f64 = d["ep_start"], d["act_f64"].astype(bool)
    all64 = [e for e in range(len(ep) - 1) if f64[ep[e]:ep[e + 1]].all()]
    all32 = [e for e in range(len(ep) - 1) if not f64[ep[e]:ep[e + 1]].any()]
    mixed = [[e] for e in range(len(ep) - 1) if e not in all64 and e not in all32]
    return [g for g in [all64, all32] + mixed if g]


def _polar_commands(amd, a, scale):
    """uavx_polar_commands on a device copy of a [n, 2] -> float64 [n, 2]"""
    import torch
    from gym_uav_collision_avoidance_amd import _lib
    L = _lib.load()
    ad = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = torch.empty((a.shape[0], 2), dtype=torch.float64, device="cuda")
    code = _lib.F64 if a.dtype == np.float64 else _lib.F32
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.uavx_polar_commands(ctypes.c_void_p(ad.data_ptr()), code, a.shape[0], ctypes.c_float(scale),
                                 ctypes.c_void_p(out.data_ptr()), stream) == 0
    torch.cuda.synchronize()
    return _np(out)


def test_conversion_kernel_float32_branch_is_exact(amd):
    """The device routine on 10^7 random float32 actions plus the edge rows (+-1, 0, -0, subnormals, NaN, +-inf): the
    trainers' float32 command bit for bit (signed zeros included; NaN where the reference gives NaN or raises)."""
    rng = np.random.default_rng(21)
    scale = float(np.linalg.norm(np.array([10.0, 10.0], F32)))
    a = np.concatenate([rng.uniform(-1, 1, (10_000_000, 2)).astype(F32), edge_actions(F32),
                        np.array([[0.3, np.inf], [0.3, -np.inf], [np.inf, 0.2]], F32)])
    got = _polar_commands(amd, a, scale)
    want = restate(a, scale).astype(np.float64)
    ok = same_bits(got, want)
    assert ok.all(), (a[~ok.all(1)][:8], got[~ok.all(1)][:8], want[~ok.all(1)][:8])


def test_conversion_kernel_float64_branch_rate(amd):
    """10^7 random float64 actions: cos / sin within 1 ulp of glibc's put every command within 2 ulps of the glibc-computed
    one (v * c rounds once more); the mismatch rate is printed (DESIGN.md section 12 quotes it)."""
    rng = np.random.default_rng(22)
    scale = 12.0
    a = np.concatenate([rng.uniform(-1, 1, (10_000_000, 2)), edge_actions(np.float64)])
    got = _polar_commands(amd, a, scale)
    want = restate(a, scale)
    fin = np.isfinite(want)
    assert (np.isnan(got) == ~fin).all()
    ulps = np.abs(got[fin] - want[fin]) / np.spacing(np.minimum(np.abs(got[fin]), np.abs(want[fin])))
    assert ulps.max() <= 2.0
    mism = ~same_bits(got, want)
    rate = dict(actions=int(a.shape[0]), x_mismatch=float(mism[:, 0].mean()), y_mismatch=float(mism[:, 1].mean()),
                any_mismatch=float(mism.any(1).mean()), max_ulp=float(ulps.max()))
    print("POLAR_REFERENCE_F64_RATE", json.dumps(rate))
    out = os.environ.get("UAVX_RATE_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(rate, f, indent=1)


def _muw_load(env, d, eps):
    n = env.num_agents
    env.set_state(loc=d["init_loc"][eps].astype(F32), vel=d["init_vel"][eps], tgt=d["init_tgt"][eps].astype(F32),
                  init_d=d["init_init_d"][eps].astype(F32), prev_d=d["init_prev_d"][eps].astype(F32), flags=d["init_flags"][eps],
                  counters=np.concatenate([d["init_counters"][eps], np.zeros((len(eps), 1), np.int64)], 1))
    assert env.num_envs == len(eps) and n == d["act"].shape[1]


def _replay_muw(amd, d, eps, polar, check):
    import torch
    ep = d["ep_start"]
    env = amd.BatchedMultiUAVWorld2D(len(eps), num_agents=d["act"].shape[1])
    _muw_load(env, d, eps)
    lens = np.array([ep[e + 1] - ep[e] for e in eps])
    diff = False
    had64 = np.zeros(len(eps), bool)    # a float64-action step ran in the episode: its velocities carry that step's ulp
    for t in range(int(lens.max())):
        live = t < lens
        rows = np.array([ep[e] + min(t, lens[k] - 1) for k, e in enumerate(eps)])
        is64 = bool(d["act_f64"][rows[live]][0])
        assert (d["act_f64"][rows[live]] == is64).all()
        a = d["act"][rows] if is64 else d["act"][rows].astype(F32)
        had64 |= is64 & live
        obs, rew, done, _ = env.step_ex(torch.from_numpy(np.ascontiguousarray(a)).cuda(), polar=polar, track_returns=False)
        st = {k: _np(v) for k, v in env.get_state().items()}
        got_obs, got_rew, got_done = _np(obs), _np(rew), _np(done)
        for k, e in enumerate(eps):
            if not live[k]:
                continue
            r = rows[k]
            same = ((st["loc"][k] == d["loc"][r].astype(F32)).all() and (st["vel"][k] == d["vel"][r]).all()
                    and (got_done[k].astype(np.uint8) == d["done"][r]).all())
            diff |= not same
            if not check:
                continue
            ctx = f"episode {e} step {t} ({'float64' if is64 else 'float32'} actions)"
            np.testing.assert_array_equal(st["loc"][k], d["loc"][r].astype(F32), err_msg=ctx + " loc")
            np.testing.assert_array_equal(st["prev_d"][k], d["prev_d"][r].astype(F32), err_msg=ctx + " prev_d")
            np.testing.assert_array_equal(st["flags"][k], d["flags"][r], err_msg=ctx + " flags")
            np.testing.assert_array_equal(got_done[k].astype(np.uint8), d["done"][r], err_msg=ctx + " done")
            if had64[k]:
                np.testing.assert_allclose(st["vel"][k], d["vel"][r], rtol=VEL64_RTOL, atol=1e-14, err_msg=ctx + " vel")
            else:
                np.testing.assert_array_equal(st["vel"][k], d["vel"][r], err_msg=ctx + " vel")
            got, want = got_obs[k].astype(np.float64), d["obs"][r].copy()
            ties = tie_agents(d["loc"][r], env.d_sense, False)
            got[ties, 4:] = 0
            want[ties, 4:] = 0
            assert obs_err(got, want) <= TOL, ctx
            assert float(np.abs(got_rew[k] - d["rew"][r]).max()) <= TOL, ctx
            if t == lens[k] - 1:   # the episode's end: the counters the trainer reads before env.reset()
                np.testing.assert_array_equal(st["counters"][k, :3], d["counters"][e], err_msg=ctx + " counters")
    env.close()
    return diff


def test_trainer_loop_replay_muw(amd):
    """Every recorded MultiUAVWorld2D(num_agents=4) episode of the trainer loop, in its own env, fed its raw actions in their
    recorded dtype with polar="reference": positions, done masks, flags, episode lengths and counters exactly,
    observations / rewards to 1e-5, velocities exactly in episodes driven by float32 actions (the policy branch) and to
    VEL64_RTOL once a float64-action (warm-up) step has run in the episode."""
    d, meta = _fixture("muw")
    for eps in _groups(d):
        _replay_muw(amd, d, eps, "reference", True)


def test_trainer_loop_fixture_tells_the_modes_apart_muw(amd):
    d, meta = _fixture("muw")
    f32_eps = [g for g in _groups(d) if not d["act_f64"][d["ep_start"][g[0]]]][0]
    assert _replay_muw(amd, d, f32_eps, True, False), "polar=True reproduced the reference fixture: it cannot tell the modes apart"


def _replay_uw(amd, d, eps, polar, check):
    import torch
    ep = d["ep_start"]
    env = amd.BatchedUAVWorld2D(len(eps))
    env.set_state(loc=d["init_loc"][eps].astype(F32), vel=d["init_vel"][eps], tgt=d["init_tgt"][eps].astype(F32),
                  init_d=d["init_init_d"][eps].astype(F32), prev_d=d["init_prev_d"][eps].astype(F32),
                  flags=np.where(d["init_vel_f32"][eps], 4, 0).astype(np.uint8),
                  counters=np.stack([d["init_steps"][eps], np.zeros(len(eps), np.int64)], 1))
    lens = np.array([ep[e + 1] - ep[e] for e in eps])
    diff = False
    had64 = np.zeros(len(eps), bool)    # a float64-action step ran in the episode: its velocities carry that step's ulp
    for t in range(int(lens.max())):
        live = t < lens
        rows = np.array([ep[e] + min(t, lens[k] - 1) for k, e in enumerate(eps)])
        is64 = bool(d["act_f64"][rows[live]][0])
        assert (d["act_f64"][rows[live]] == is64).all()
        a = d["act"][rows] if is64 else d["act"][rows].astype(F32)
        had64 |= is64 & live
        obs, rew, done, info = env.step_ex(torch.from_numpy(np.ascontiguousarray(a)).cuda(), polar=polar, track_returns=False)
        st = {k: _np(v) for k, v in env.get_state().items()}
        got_obs, got_rew, got_done, got_dist = _np(obs), _np(rew), _np(done), _np(info["distance"])
        for k, e in enumerate(eps):
            if not live[k]:
                continue
            r = rows[k]
            diff |= not ((st["loc"][k] == d["loc"][r].astype(F32)).all() and (st["vel"][k] == d["vel"][r]).all())
            if not check:
                continue
            ctx = f"episode {e} step {t} ({'float64' if is64 else 'float32'} actions)"
            assert bool(got_done[k]) == bool(d["done"][r]), ctx
            np.testing.assert_array_equal(st["loc"][k], d["loc"][r].astype(F32), err_msg=ctx + " loc")
            if had64[k]:
                np.testing.assert_allclose(st["vel"][k], d["vel"][r], rtol=VEL64_RTOL, atol=1e-14, err_msg=ctx + " vel")
            else:
                np.testing.assert_array_equal(st["vel"][k], d["vel"][r], err_msg=ctx + " vel")
            assert obs_err(got_obs[k], d["obs"][r], (1, 3)) <= TOL, ctx
            r_ref = d["rew"][r]
            assert abs(float(got_rew[k]) - r_ref) <= max(TOL, float(np.spacing(F32(abs(r_ref))))), ctx
            assert float(got_dist[k]) == float(F32(d["distance"][r])), ctx
            if t == lens[k] - 1:
                assert int(st["counters"][k, 0]) == int(d["counters"][e, 0]), ctx
    env.close()
    return diff


def test_trainer_loop_replay_uw(amd):
    """The same for UAVWorld2D (test_sac.py:68-110): the float32 command of a float32 action takes the float32 command's
    arithmetic in the step (act_f32), the float64 one the float64 arithmetic."""
    d, meta = _fixture("uw")
    for eps in _groups(d):
        _replay_uw(amd, d, eps, "reference", True)


def test_trainer_loop_fixture_tells_the_modes_apart_uw(amd):
    d, meta = _fixture("uw")
    f32_eps = [g for g in _groups(d) if not d["act_f64"][d["ep_start"][g[0]]]][0]
    assert _replay_uw(amd, d, f32_eps, True, False)


def _actions32(rng, E, n):
    a = rng.uniform(-1, 1, (E, n, 2)).astype(F32)
    edge = edge_actions(F32)
    edge = edge[np.isfinite(edge).all(1)]
    m = min(len(edge), E)
    a[:m, 0] = edge[:m]                        # one edge row per env among the first ones (agent 0)
    return a


@pytest.mark.parametrize("E,n,tiles,bodies,policy,code,cap,T", [
    (65536, 4, None, 0, "agent0_done", 1, 30, 40),
    (4096, 8, None, 0, "agent0_done", 1, 25, 60),
    (4096, 8, "2", 0, "agent0_done", 1, 25, 60),
    (2048, 8, None, 16, "agent0_done", 1, 20, 50),
    (1531, 5, None, 0, "all_done", 2, 20, 60),
])
def test_step_ex_reference_vs_oracle_cartesian(amd, oracle_mod, monkeypatch, E, n, tiles, bodies, policy, code, cap, T):
    """Full batches stepped with polar="reference" on float32 actions (edge rows mixed in) == the oracle's CARTESIAN step
    fed the host restatement's float32 commands: state, done, reset / ended / truncated, counters and episode statistics
    bit for bit, observations and rewards to 1e-5."""
    import torch
    if tiles:
        monkeypatch.setenv("UAVX_TILES", tiles)
    kw = dict(x_size=26.0, y_size=26.0, num_agents=n, d_sense=9.0, **(dict(num_bodies=bodies, body_period=8) if bodies else {}))
    env = amd.BatchedMultiUAVWorld2D(E, seed=13, env_offset=2, **kw)
    orc = oracle_mod.OracleMulti(num_envs=E, nthreads=16, **kw)
    env.reset()
    orc.reset_philox(13, env_offset=2)
    scale = float(np.linalg.norm(np.array([10.0, 10.0], F32)))
    rng = np.random.default_rng(5)
    resets = 0
    for t in range(T):
        a = _actions32(rng, E, n)
        cmd = restate(a, scale).astype(np.float64)
        og, rg, dg, info = env.step_ex(torch.from_numpy(a).cuda(), polar="reference", auto_reset=policy, step_cap=cap,
                                       track_returns=True)
        oo, ro, do, rm, en, tr = orc.step_ex(cmd, reset_policy=code, step_cap=cap, track_returns=True, seed=13, env_offset=2,
                                             with_end=True)
        ctx = f"step {t}"
        np.testing.assert_array_equal(_np(info["reset_mask"]).astype(np.uint8), rm, err_msg=ctx)
        np.testing.assert_array_equal(_np(info["ended"]).astype(np.uint8), en, err_msg=ctx)
        np.testing.assert_array_equal(_np(info["truncated"]).astype(np.uint8), tr, err_msg=ctx)
        np.testing.assert_array_equal(_np(dg).astype(np.uint8), do, err_msg=ctx)
        st, ref = env.get_state(), orc.get_state()
        for key in ("loc", "vel", "tgt", "init_d", "prev_d", "flags"):
            np.testing.assert_array_equal(_np(st[key]), ref[key], err_msg=f"{ctx} {key}")
        np.testing.assert_array_equal(_np(st["counters"]), ref["counters"].astype(np.int32), err_msg=ctx)
        assert obs_err(_np(og), oo) <= TOL and float(np.abs(_np(rg) - ro).max()) <= TOL, ctx
        resets += int(rm.sum())
    assert resets > 0
    stats = {k: _np(v) for k, v in env.episode_stats().items()}
    np.testing.assert_array_equal(stats["episodes"], orc.fin_counts[:, 0])
    np.testing.assert_array_equal(stats["steps"], orc.fin_counts[:, 1])
    np.testing.assert_array_equal(stats["reach"], orc.fin_counts[:, 2])
    np.testing.assert_array_equal(stats["coll"], orc.fin_counts[:, 3])
    assert int(env.nonfinite_count().sum()) == 0
    env.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float64_positions_reference_vs_cartesian_twin(amd, dtype):
    """Float64-position mode (reset_circular, step64_ref_kernel): polar="reference" == a twin batch stepped with the
    restatement's commands through the cartesian float64-position path.  Bit for bit with float32 actions; with float64
    actions the twin is fed the device conversion's own commands (uavx_polar_commands), so the check is exact too."""
    import torch
    E, n, T = 4096, 6, 80
    a_env = amd.BatchedMultiUAVWorld2D(E, num_agents=n, seed=3)
    b_env = amd.BatchedMultiUAVWorld2D(E, num_agents=n, seed=3)
    a_env.reset_circular()
    b_env.reset_circular()
    assert a_env.position_mode == "float64"
    scale = float(np.linalg.norm(np.array([10.0, 10.0], F32)))
    rng = np.random.default_rng(9)
    for t in range(T):
        a = rng.uniform(-1, 1, (E, n, 2)).astype(dtype)
        if dtype == np.float32:
            cmd = restate(a, scale).astype(np.float64)
        else:
            cmd = _polar_commands(amd, a.reshape(-1, 2), scale).reshape(E, n, 2)
            want = restate(a, scale)
            assert (np.abs(cmd - want) <= 2 * np.spacing(np.minimum(np.abs(cmd), np.abs(want)))).all()
        oa, ra, da, _ = a_env.step_ex(torch.from_numpy(a).cuda(), polar="reference")
        ob, rb, db, _ = b_env.step_ex(torch.from_numpy(cmd).cuda(), polar=False)
        for k in ("loc", "tgt", "prev_d"):
            assert torch.equal(a_env.get_state_f64()[k], b_env.get_state_f64()[k]), (t, k)
        assert torch.equal(a_env.get_state()["vel"], b_env.get_state()["vel"]), t
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), t
    a_env.close()
    b_env.close()


@pytest.mark.parametrize("cap", [0, 60])
def test_uw_step_ex_reference_vs_oracle_cartesian(amd, oracle_mod, cap):
    """UAVWorld2D at 65 536 envs: polar="reference" on float32 actions == the oracle's cartesian step fed the restatement's
    FLOAT32 commands (the first-step float32 arithmetic included), with auto-reset."""
    import torch
    E = 65536
    env = amd.BatchedUAVWorld2D(E, seed=31, env_offset=9)
    orc = oracle_mod.OracleSingle(num_envs=E, nthreads=16)
    env.reset()
    orc.reset_philox(31, env_offset=9)
    rng = np.random.default_rng(6)
    for t in range(70):
        a = rng.uniform(-1, 1, (E, 2)).astype(F32)
        edge = edge_actions(F32)
        edge = edge[np.isfinite(edge).all(1)]
        a[:len(edge)] = edge
        cmd = restate(a, 12.0)
        assert cmd.dtype == F32
        og, rg, dg, info = env.step_ex(torch.from_numpy(a).cuda(), polar="reference", auto_reset=True, step_cap=cap)
        oo, ro, do, io, rm = orc.step_ex(cmd, polar=False, auto_reset=True, step_cap=cap, seed=31, env_offset=9)
        ctx = f"step {t}"
        np.testing.assert_array_equal(_np(info["reset_mask"]).astype(np.uint8), rm, err_msg=ctx)
        np.testing.assert_array_equal(_np(dg).astype(np.uint8), do, err_msg=ctx)
        st = env.get_state()
        np.testing.assert_array_equal(_np(st["loc"]), orc.loc.astype(F32), err_msg=ctx)
        np.testing.assert_array_equal(_np(st["vel"]), orc.vel, err_msg=ctx)
        np.testing.assert_array_equal(_np(st["counters"])[:, 0], orc.steps, err_msg=ctx)
        assert obs_err(_np(og), oo, (1, 3)) <= TOL, ctx
        tol_r = np.maximum(TOL, np.spacing(np.abs(ro).astype(F32)).astype(np.float64))
        assert (np.abs(_np(rg) - ro) <= tol_r).all(), ctx
    env.close()


def test_vector_env_reference_mode(amd):
    """UAVVectorEnv(polar="reference") keeps the option (not bool()-ed into polar=True), keeps the [-1, 1] float32 action box,
    and each step is the one fused launch: trajectories equal a batch driven with step_ex(polar="reference")."""
    import torch
    from gym_uav_collision_avoidance_amd import UAVSingleVectorEnv, UAVVectorEnv
    E, n = 640, 4
    venv = UAVVectorEnv(E, num_agents=n, step_cap=50, polar="reference", seed=21)
    twin = amd.BatchedMultiUAVWorld2D(E, num_agents=n, seed=21)
    assert venv.polar == "reference" and float(venv.action_space.high.max()) == 1.0 and venv.action_space.dtype == np.float32
    venv.reset(seed=21)
    twin.reset(seed=21)
    rng = np.random.default_rng(2)
    for t in range(60):
        a = torch.from_numpy(rng.uniform(-1, 1, size=(E, n, 2)).astype(F32)).cuda()
        og, rg, dg, info = venv.step(a)
        ot, rt, dt, it = twin.step_ex(a, polar="reference", auto_reset="agent0_done", step_cap=50)
        assert torch.equal(og, ot) and torch.equal(rg, rt) and torch.equal(dg, dt), t
    venv.close()
    twin.close()
    sv = UAVSingleVectorEnv(256, seed=4, step_cap=40, polar="reference")
    assert sv.polar == "reference" and sv.single_action_space.shape == (2,)
    sv.reset()
    o, r, d, info = sv.step(torch.zeros((256, 2), dtype=torch.float32, device=sv.device))
    assert torch.isfinite(o).all()
    sv.close()
    with pytest.raises(ValueError):
        UAVVectorEnv(8, polar="float32")


def test_device_replay_graph_capture_with_fused_actor(amd):
    """DeviceReplay.step(polar="reference") fed by FusedActor.act(..., out=mem.action_slot()): captured in a graph and
    replayed == eager execution, bit for bit."""
    import torch
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.fused_actor import FusedActor
    from gym_uav_collision_avoidance_amd.policy import GaussianPolicy
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    RING, kw = 4, dict(polar="reference", auto_reset="agent0_done", step_cap=30)
    torch.manual_seed(3)
    fa = FusedActor(GaussianPolicy(10, 2, hidden=256).cuda())
    loops = []
    for _ in range(2):
        env = BatchedMultiUAVWorld2D(256, num_agents=4, seed=21)
        mem = DeviceReplay(env, horizon=RING - 1)
        mem.begin(env.reset())

        def one_pass(mem=mem):
            for _ in range(RING):
                fa.act(mem.state, out=mem.action_slot())
                mem.step(**kw)
        one_pass()
        loops.append((env, mem, one_pass))
    env_e, mem_e, pass_e = loops[0]
    pass_e()
    pass_e()
    env_g, mem_g, pass_g = loops[1]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pass_g()
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for f in ("obs", "act", "rew", "done"):
        assert torch.equal(getattr(mem_e, f), getattr(mem_g, f)), f
    assert torch.equal(env_e.get_state()["vel"], env_g.get_state()["vel"])
    env_e.close()
    env_g.close()


def test_rollout_trajectories_reference_mode(amd):
    """rollout_trajectories(polar="reference") on the circular layout runs in float64-position mode (step64_ref_kernel)."""
    import torch
    from gym_uav_collision_avoidance_amd.evaluate import rollout_trajectories

    def policy_fn(obs):
        return torch.stack([torch.full_like(obs[..., 0], 0.2), obs[..., 3]], -1).to(torch.float32)

    out = rollout_trajectories(policy_fn, 4, episodes=8, max_steps=120, circular=True, polar="reference")
    assert out["positions"].dtype == torch.float64
    assert torch.isfinite(out["positions"]).all()
    moved = (out["positions"][-1] - out["positions"][0]).abs().sum()
    assert float(moved) > 0

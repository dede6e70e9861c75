"""The tail of the 4-UAV one-step kernel (csrc/uavx_multi_step.hpp: UAVX_TAILCOLD, UAVX_DONEROW).

  * flags-word change, arrival, hard collision and non-finite reward share one wave-uniform test and one cold block: a
    wavefront that has all of them in one launch must raise all of their counters;
  * the env's four done bytes leave as one dword from the quad's first lane, with the reward row: a caller's done array that
    is not 4-byte aligned gets byte stores, and nothing outside the array is touched;
  * the wavefront's step counter: every launch must count exactly once, whatever ran between two launches (step_k, a masked
    reset, a replayed graph).

Plain `step`, N = 4, against the CPU oracle at E = 1 (one live quad), 15 (partial wavefront), 16 (exact), 17 (two workgroups,
one quad in the second), 33 (three workgroups); float32 and float64 commands; the small box of test_gpu_packed_rows.py, where
arrivals and collisions happen.  State, dones, flags and counters bit for bit, rewards and observations at the parity tests' 1e-5."""
import numpy as np
import pytest

from golden_util import obs_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
N = 4
STEPS = 64
KW = dict(x_size=12.0, y_size=10.0, num_agents=N, d_sense=9.0, collider_radius=0.5)   # small box: collisions, arrivals
DONE_SENTINEL = 0xA5


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import gym_uav_collision_avoidance_amd as pkg
    return pkg


def _np(t):
    return t.detach().cpu().numpy()


def _commands(rng, orc, dtype):
    """Velocity commands along a noisy bearing to the target at a noisy speed (the oracle's state is the device's bit for bit)."""
    d = orc.tgt - orc.loc
    v = np.hypot(d[..., 0], d[..., 1]) * rng.uniform(0.2, 3.0, size=d.shape[:2])
    th = np.arctan2(d[..., 1], d[..., 0]) + rng.normal(0.0, 0.4, size=d.shape[:2])
    # every fifth slot flees at full speed: it leaves the box and reports done from then on (not under evaluate), so the done
    # bytes of a quad are a mix of 0 and 1 in a lane that moves from env to env
    flee = (np.arange(d.shape[0] * d.shape[1]).reshape(d.shape[:2]) % 5) == 3
    th, v = np.where(flee, th + np.pi, th), np.where(flee, 10.0, v)
    return np.stack([v * np.cos(th), v * np.sin(th)], axis=-1).astype(dtype)


def _pair(amd, oracle_mod, E, seed):
    env = amd.BatchedMultiUAVWorld2D(E, seed=seed, env_offset=7, **KW)
    orc = oracle_mod.OracleMulti(num_envs=E, nthreads=4, **KW)
    env.reset()
    orc.reset_philox(seed, mask=None, env_offset=7)
    return env, orc


def _check_state(env, orc, ctx):
    """State and flags bit for bit; steps, reach and coll of metrics() equal to the oracle's."""
    ref = orc.get_state()
    st = {k: _np(v) for k, v in env.get_state().items()}
    np.testing.assert_array_equal(st["loc"], ref["loc"], err_msg=ctx + " loc")
    np.testing.assert_array_equal(st["vel"], ref["vel"], err_msg=ctx + " vel")
    np.testing.assert_array_equal(st["flags"], ref["flags"], err_msg=ctx + " flags")
    np.testing.assert_array_equal(_np(env.metrics())[:, :3], orc.counters[:, :3].astype(np.int32), err_msg=ctx + " steps/reach/coll")


def _check_outputs(got, want, ctx):
    obs_g, rew_g, done_g = got
    obs_o, rew_o, done_o = want
    np.testing.assert_array_equal(_np(done_g).astype(np.uint8), done_o, err_msg=ctx + " dones")
    e_obs = obs_err(_np(obs_g), obs_o)
    e_rew = float(np.abs(_np(rew_g) - rew_o).max())
    assert e_obs <= TOL and e_rew <= TOL, f"{ctx}: obs err {e_obs:.3g}, rew err {e_rew:.3g}"


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("E", [1, 15, 16, 17, 33])
def test_tail_against_oracle(amd, oracle_mod, E, dtype):
    import torch
    env, orc = _pair(amd, oracle_mod, E, seed=5100 + E)
    rng = np.random.default_rng(200 * E + (dtype is np.float64))
    dones = 0
    for t in range(STEPS):
        act = _commands(rng, orc, dtype)
        ev = bool(t % 5 == 4)
        got = env.step(torch.from_numpy(act).to(env.device) if dtype is np.float32 else act, evaluate=ev)[:3]
        ctx = f"E={E} {np.dtype(dtype).name} step {t}"
        want = orc.step(act, evaluate=ev)
        _check_outputs(got, want, ctx)
        _check_state(env, orc, ctx)
        dones += int(want[2].sum())
    assert 0 < dones < STEPS * E * N, "the done bytes must be a mix of 0 and 1"
    assert (orc.counters[:, 0] == STEPS).all()
    assert orc.flags.any() or E == 1, "the batch must set flags (collisions, arrivals)"
    env.close()


@pytest.mark.parametrize("E", [1, 17, 33])
def test_step_counter_through_step_k_and_masked_reset(amd, oracle_mod, E):
    """step x 3, step_k(K = 4), step x 2, reset(mask), step x 2: the step launch finds the count the launch before it left,
    whichever kernel that was, and a reset env starts from 0 while its wavefront's word goes on counting."""
    import torch
    seed = 5200 + E
    env, orc = _pair(amd, oracle_mod, E, seed=seed)
    rng = np.random.default_rng(300 + E)

    def one(tag):
        act = _commands(rng, orc, np.float32)
        got = env.step(torch.from_numpy(act).to(env.device))[:3]
        _check_outputs(got, orc.step(act), f"E={E} {tag}")
        _check_state(env, orc, f"E={E} {tag}")

    for t in range(3):
        one(f"step {t}")
    tape = []
    for k in range(4):   # the oracle runs ahead through the tape; the device takes it in one launch
        tape.append(_commands(rng, orc, np.float32))
        want = orc.step(tape[-1])
    got = env.step_k(np.stack(tape))[:3]
    _check_outputs(got, want, f"E={E} step_k")
    _check_state(env, orc, f"E={E} step_k")
    for t in range(2):
        one(f"step {t} after step_k")
    mask = (np.arange(E) % 3 == 0)
    env.reset(mask=torch.from_numpy(mask).to(env.device))
    orc.reset_philox(seed, mask=mask, env_offset=7)
    _check_state(env, orc, f"E={E} masked reset")
    for t in range(2):
        one(f"step {t} after reset")
    want_steps = np.where(mask, 2, 11)
    np.testing.assert_array_equal(_np(env.metrics())[:, 0], want_steps)
    env.close()


def test_step_counter_in_a_replayed_graph(amd, oracle_mod):
    """Three `step` nodes captured once and replayed twice count six steps, like six eager launches of the same commands."""
    import torch
    E = 17
    env_g, orc = _pair(amd, oracle_mod, E, seed=5300)
    env_e, _ = _pair(amd, oracle_mod, E, seed=5300)
    rng = np.random.default_rng(53)
    act = torch.from_numpy(_commands(rng, orc, np.float32)).to(env_g.device)   # one command, held: six steps towards the targets
    side = torch.cuda.Stream(env_g.device)
    side.wait_stream(torch.cuda.current_stream(env_g.device))
    with torch.cuda.stream(side):      # lazy initialisation outside the capture, on a scratch batch
        scratch, _ = _pair(amd, oracle_mod, E, seed=5301)
        scratch.step(act)
    torch.cuda.current_stream(env_g.device).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(3):
            out_g = env_g.step(act)
    assert int(_np(env_g.metrics())[:, 0].max()) == 0, "a capture launches nothing"
    for _ in range(2):
        g.replay()
    for _ in range(6):
        out_e = env_e.step(act)
        orc.step(_np(act))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(env_g.metrics()), _np(env_e.metrics()))
    assert (_np(env_g.metrics())[:, 0] == 6).all()
    _check_state(env_g, orc, "graph")
    _check_state(env_e, orc, "eager")
    for a, b in zip(out_g[:3], out_e[:3]):
        np.testing.assert_array_equal(_np(a).view(np.uint8), _np(b).view(np.uint8))
    for e in (env_g, env_e, scratch):
        e.close()


def test_one_wavefront_raises_every_rare_counter_in_one_launch(amd, oracle_mod):
    """An arrival (env 0), a hard collision (env 1) and a poked NaN velocity (env 2) in the same wavefront and the same launch:
    reach, coll and the non-finite tripwire all count, the flags words are stored, and the step is counted once."""
    E = 16   # one wavefront
    env, orc = _pair(amd, oracle_mod, E, seed=5400)
    st = orc.get_state()
    loc, tgt, vel = st["loc"].copy(), st["tgt"].copy(), np.zeros_like(st["vel"])
    corners = np.array([[2.0, 2.0], [8.0, 2.0], [2.0, 7.0], [8.0, 7.0]], np.float32)
    loc[0] = corners; tgt[0] = corners + np.float32(3.0) * np.array([[0, 1], [0, 1], [0, -1], [0, -1]], np.float32)
    tgt[0, 0] = loc[0, 0] + np.array([0.2, 0.0], np.float32)        # at rest 0.2 m from its target: arrives
    loc[1] = corners; loc[1, 1] = loc[1, 0] + np.array([0.1, 0.0], np.float32)   # 0.1 m apart: hard collision
    tgt[1] = loc[1] + np.float32(3.0)
    vel[2, 0] = [np.nan, 0.0]
    d = tgt - loc
    prev_d = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float32)
    flags = np.zeros((E, N), np.uint8)
    for side in (env, orc):
        side.set_state(loc=loc, vel=vel, tgt=tgt, init_d=prev_d, prev_d=prev_d, flags=flags)
    act = np.zeros((E, N, 2), np.float32)
    got = env.step(act)[:3]
    obs_o, rew_o, done_o = orc.step(act)
    assert orc.counters[0, 1] >= 1 and orc.counters[1, 2] >= 1 and not np.isfinite(rew_o[2, 0]), "scenario: arrival, collision, NaN"
    np.testing.assert_array_equal(_np(got[2]).astype(np.uint8), done_o)
    fin = np.isfinite(rew_o)
    assert float(np.abs(_np(got[1])[fin] - rew_o[fin]).max()) <= TOL and np.isnan(_np(got[1])[~fin]).all()
    _check_state(env, orc, "rare block")
    np.testing.assert_array_equal(_np(env.nonfinite_count()), (~fin).sum(axis=1))
    assert (_np(env.metrics())[:, 0] == 1).all()
    env.close()


@pytest.mark.parametrize("E", [1, 17])
def test_done_array_at_byte_offset_one(amd, oracle_mod, E):
    """A caller's done tensor one byte into its buffer takes byte stores: bit-equal to the aligned run, sentinels on both
    sides untouched (also those that share the first and the last dword with the array)."""
    import torch
    env_a, orc = _pair(amd, oracle_mod, E, seed=5500 + E)   # (the oracle only steers the commands here)
    env_u, _ = _pair(amd, oracle_mod, E, seed=5500 + E)
    dev, n = env_a.device, E * N
    big = {k: torch.full((16 + n + 16,), DONE_SENTINEL, dtype=torch.uint8, device=dev) for k in "au"}
    lead = {"a": 16, "u": 17}
    done = {k: big[k][lead[k]:lead[k] + n].view(E, N) for k in "au"}
    assert done["a"].data_ptr() % 4 == 0 and done["u"].data_ptr() % 4 == 1
    obs = {k: torch.empty((E, N, 10), dtype=torch.float32, device=dev) for k in "au"}
    rew = {k: torch.empty((E, N), dtype=torch.float32, device=dev) for k in "au"}
    rng = np.random.default_rng(55 + E)
    seen = 0
    for t in range(STEPS):
        act = _commands(rng, orc, np.float32)
        orc.step(act)
        env_a.step(act, out=(obs["a"], rew["a"], done["a"]))
        env_u.step(act, out=(obs["u"], rew["u"], done["u"]))
        ctx = f"E={E} step {t}"
        for k in "au":
            b = _np(big[k])
            assert (b[:lead[k]] == DONE_SENTINEL).all() and (b[lead[k] + n:] == DONE_SENTINEL).all(), ctx + ": done sentinel overwritten"
        np.testing.assert_array_equal(_np(done["u"]), _np(done["a"]), err_msg=ctx + " dones")
        np.testing.assert_array_equal(_np(rew["u"]).view(np.uint32), _np(rew["a"]).view(np.uint32), err_msg=ctx + " rewards")
        np.testing.assert_array_equal(_np(obs["u"]).view(np.uint32), _np(obs["a"]).view(np.uint32), err_msg=ctx + " obs")
        np.testing.assert_array_equal(_np(env_u.metrics()), _np(env_a.metrics()), err_msg=ctx + " counters")
        seen += int(_np(done["a"]).sum())
    assert seen > 0, "no done byte was ever set"
    env_a.close()
    env_u.close()

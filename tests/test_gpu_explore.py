"""The exploration launch (include/uavx_explore.h, gym_uav_collision_avoidance_amd/exploration.py) on the
MI355X: bit-equal to the forward's own SAC_SAMPLE / ADD_CLAMP epilogues on fed and on drawn normals, the drawn normals
against the float64 restatement (tests/explore_ref.py), DDPG's Ornstein-Uhlenbeck value against the reference's own runs
(tests/golden/ou_reference.npz), warm-up and random actions, shard cuts, reset flags, strided output, graph replay and the
learners' select_action(explore=...)."""
import os

import numpy as np
import pytest
import torch

import explore_ref as er
from fused_ref import heads as _heads
from gym_uav_collision_avoidance_amd import _actor_lib, policy
from gym_uav_collision_avoidance_amd._fused_common import stream

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROWS = (1, 63, 64, 65, 257)     # a partial wavefront, a whole one, a partial workgroup, a second workgroup
ACTORS = {"sac": policy.GaussianPolicy, "td3": policy.TD3Actor, "ddpg": policy.DDPGActor}
KIND = {"sac": er.SAC, "td3": er.TD3, "ddpg": er.DDPG}
BIG_OFFSET = 2 ** 40 + 3
_cache = {}


def _actor(name, precision="f32"):
    """One packed actor per (kind, precision) for the whole module: the tests only read it."""
    if (name, precision) not in _cache:
        from gym_uav_collision_avoidance_amd.fused_actor import FusedActor
        torch.manual_seed(31 + len(name))
        _cache[name, precision] = FusedActor.from_module(ACTORS[name]().to(DEV).eval(), precision=precision)
    return _cache[name, precision]


def _explore(name, rows, precision="f32", **kw):
    from gym_uav_collision_avoidance_amd.exploration import Exploration
    return Exploration(_actor(name, precision), rows, **kw)


def _obs(rows, seed=1):
    return torch.rand((rows, 10), generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV) * 2 - 1


def _forward(fa, obs, eps32, scale=0.1):
    """The forward's own exploration epilogue on fed float32 noise."""
    mode = _actor_lib.SAC_SAMPLE if fa.kind == _actor_lib.SAC else _actor_lib.ADD_CLAMP
    out = torch.empty((obs.shape[0], 2), dtype=torch.float32, device=DEV)
    return fa._launch(obs, eps32.contiguous(), scale, mode, out, 2)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _state(ex):
    s = ex.state.cpu().numpy()
    return s[:, 0].copy(), s.view(np.uint32)[:, 2].copy(), s.view(np.uint32)[:, 3].copy()


# ---- 1. fed normals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["sac", "td3"])
def test_fed_normals_equal_the_forwards_own_epilogue(name, precision):
    fa = _actor(name, precision)
    for rows in ROWS:
        ex = _explore(name, rows, precision, seed=3)
        obs = _obs(rows, seed=rows)
        eps = torch.randn((rows, 2), generator=torch.Generator(device=DEV).manual_seed(rows), device=DEV)
        eps[0, 0] = 0.0
        used = torch.full((rows, 2), 7.0, dtype=torch.float64, device=DEV)
        got = ex.act(obs, normals=eps.double(), normals_out=used)
        assert _same(got, _forward(fa, obs, eps)), (name, precision, rows)
        assert _same(used, eps.double())
        assert not _same(got, fa.act(obs))                   # the noise arrived
        x, n, res = _state(ex)
        assert (x == 0).all() and (n == 1).all() and (res == 0).all()


# ---- 2. drawn normals -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sac", "td3"])
def test_drawn_normals_meet_the_restatement_and_drive_the_forwards_epilogue(name):
    fa, seed, off = _actor(name), 0x1234567887654321, 5
    worst = 0.0
    for rows in ROWS:
        ex = _explore(name, rows, seed=seed, row_offset=off)
        obs = _obs(rows, seed=40 + rows)
        used = torch.zeros((rows, 2), dtype=torch.float64, device=DEV)
        for call in range(2):
            got = ex.act(obs, normals_out=used)
            w = er.words(seed, np.arange(rows, dtype=np.uint64) + np.uint64(off), call, 0)
            want = np.stack(er.normals(w[0], w[1]), axis=1)
            err = float(np.abs(used.cpu().numpy() - want).max())
            worst = max(worst, err)
            assert err <= 1e-12, (name, rows, call, err)
            assert _same(got, _forward(fa, obs, used.float())), (name, rows, call)
    print(name, "largest |normals_out - restatement|", worst)


# ---- 3. DDPG against the reference's OU runs --------------------------------------------------------------------------
@pytest.mark.parametrize("case,rows", [(0, 1), (0, 63), (0, 64), (0, 65), (0, 257), (1, 257), (2, 257)])
def test_ddpg_follows_the_reference_ou_runs(case, rows):
    _, fx = er.load_fixture(GOLDEN)
    z, xs, sigma = fx[f"case{case}_normals"], fx[f"case{case}_x"], er.OU_CASES[case][1]
    fa = _actor("ddpg")
    ex = _explore("ddpg", rows, seed=9, ou_sigma=sigma)
    ex.state.view(torch.int32)[:, 3] = 0x5A5A5A5A               # the reserved word: carried, never changed
    obs = _obs(rows, seed=70 + rows)
    det = fa.act(obs).cpu().numpy().astype(np.float64)
    fed = torch.zeros((rows, 2), dtype=torch.float64, device=DEV)
    for k in range(64):
        fed[:, 0] = float(z[k])
        fed[:, 1] = -float(z[k])                                # not read by DDPG
        got = ex.act(obs, normals=fed).cpu().numpy()
        x, n, res = _state(ex)
        assert np.array_equal(x, np.full(rows, xs[k])), (case, rows, k)
        assert (n == k + 1).all() and (res == 0x5A5A5A5A).all()
        want = np.clip(det + xs[k], -1.0, 1.0).astype(np.float32)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (case, rows, k)


# ---- 4. warm-up and random actions ------------------------------------------------------------------------------------
def _raw(fa, obs):
    r = fa.raw(obs)
    return (torch.cat(r, dim=-1) if isinstance(r, tuple) else r).cpu().numpy()


def _check_against_restatement(name, ex, obs, n0, x0, p, warmup):
    """One act() from call counts n0 and OU values x0: random rows are the restatement's, exactly; the others equal the
    forward's epilogue fed the normals the launch reports (SAC / TD3) or the OU formula (DDPG)."""
    fa, rows = ex.actor, ex.rows
    ex.steps.copy_(torch.from_numpy(n0.astype(np.int32)).to(DEV))
    ex.ou_state.copy_(torch.from_numpy(x0).to(DEV))
    used = torch.zeros((rows, 2), dtype=torch.float64, device=DEV)
    got = ex.act(obs, normals_out=used).cpu().numpy()
    det = fa.act(obs).cpu().numpy()
    a, x1, n1, rnd, nz = er.act(KIND[name], _raw(fa, obs), x0, n0.astype(np.uint32), ex.seed, row_offset=ex.row_offset,
                                warmup_steps=warmup, p=p, noise_std=ex.noise_std, sigma=ex.ou_sigma,
                                fed=used.cpu().numpy(), tanh32=det)
    x, n, _ = _state(ex)
    assert np.array_equal(n, n1) and np.array_equal(x, x1)
    assert np.array_equal(x[rnd], x0[rnd])                      # a random action leaves the OU value alone
    if name == "ddpg":
        assert (x[~rnd] != x0[~rnd]).all()
        assert np.array_equal(got.view(np.int32), a.astype(np.float32).view(np.int32))
    else:
        fwd = _forward(fa, obs, used.float(), ex.noise_std).cpu().numpy()
        assert np.array_equal(got[rnd].view(np.int32), a[rnd].astype(np.float32).view(np.int32))
        assert np.array_equal(got[~rnd].view(np.int32), fwd[~rnd].view(np.int32))
    assert np.isfinite(got).all() and (np.abs(got) <= 1).all()
    return rnd


@pytest.mark.parametrize("name", sorted(ACTORS))
def test_warmup_boundary_and_random_actions(name):
    warmup = 5
    for rows in ROWS:
        ex = _explore(name, rows, seed=77, row_offset=1000, warmup_steps=warmup, ou_sigma=0.3)
        obs = _obs(rows, seed=90 + rows)
        n0 = np.where(np.arange(rows) % 2 == 0, warmup - 1, warmup).astype(np.uint32)
        x0 = np.linspace(0.25, 0.75, rows)
        rnd = _check_against_restatement(name, ex, obs, n0, x0, 0.0, warmup)
        assert np.array_equal(rnd, n0 < warmup)                 # the two sides of the boundary


@pytest.mark.parametrize("name", sorted(ACTORS))
def test_random_probability_by_value_and_from_the_device_slot(name):
    from gym_uav_collision_avoidance_amd.exploration import launch
    rows = 257
    obs = _obs(rows, seed=5)
    n0, x0 = np.full(rows, 11, dtype=np.uint32), np.linspace(-0.5, 0.5, rows)
    for p in (0.0, 1.0, 0.5):
        ex = _explore(name, rows, seed=123, random_prob=p, ou_sigma=0.3)
        rnd = _check_against_restatement(name, ex, obs, n0, x0, p, 0)
        if p != 0.5:
            assert rnd.all() == bool(p) and rnd.any() == bool(p)
        else:
            assert 64 < int(rnd.sum()) < 192                    # 128.5 +- 8 sigma
        # by value, through the ABI, from the same state: the same bits
        ex.steps.fill_(11)
        ex.ou_state.copy_(torch.from_numpy(x0).to(DEV))
        slot_out, slot_state = ex.act(obs).clone(), ex.state.clone()
        ex.steps.fill_(11)
        ex.ou_state.copy_(torch.from_numpy(x0).to(DEV))
        out = torch.empty((rows, 2), dtype=torch.float32, device=DEV)
        rc = launch(ex._lib, stream(ex.device), kind=ex.kind, rows=rows, seed=ex.seed, raw=ex._raw.data_ptr(),
                    raw_stride=ex._cols, out=out.data_ptr(), out_stride=2, state=ex.state.data_ptr(), random_prob=p,
                    noise_std=ex.noise_std, ou_sigma=ex.ou_sigma, ou_theta=ex.ou_theta, ou_dt=ex.ou_dt)
        assert rc == _actor_lib.OK
        assert _same(out, slot_out) and _same(ex.state, slot_state)
    # annealing: the slot is read by the launch, not by the call
    ex = _explore(name, rows, seed=123, random_prob=0.0)
    first = ex.act(obs).clone()
    ex.steps.zero_()
    ex.ou_state.zero_()
    ex.set_random_prob(1.0)
    w = er.words(123, np.arange(rows, dtype=np.uint64), 0, 0)
    want = np.stack([er.uniform_action(w[2]), er.uniform_action(w[3])], axis=1)
    assert np.array_equal(ex.act(obs).cpu().numpy().view(np.int32), want.view(np.int32)) and not _same(first, ex.act(obs))


# ---- 5. shard cuts and big offsets ------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, BIG_OFFSET])
@pytest.mark.parametrize("name", sorted(ACTORS))
def test_two_shards_equal_one_batch(name, offset):
    R, h = 257, 128
    kw = dict(seed=0xFEDCBA9876543210, warmup_steps=1, random_prob=0.5, ou_sigma=0.4)
    whole = _explore(name, R, row_offset=offset, **kw)
    parts = (_explore(name, h, row_offset=offset, **kw), _explore(name, R - h, row_offset=offset + h, **kw))
    moved = _explore(name, R, row_offset=offset + 1, **kw)
    obs = _obs(R, seed=17)
    for call in range(3):
        a = whole.act(obs)
        b = torch.cat([parts[0].act(obs[:h]), parts[1].act(obs[h:])])
        assert _same(a, b), (name, offset, call)
        assert _same(whole.state, torch.cat([parts[0].state, parts[1].state]))
        assert not _same(a, moved.act(obs))                     # the draws belong to the global row
    assert (_state(whole)[1] == 3).all()


# ---- 6. reset flags ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("rows,per_env", [(64, 4), (63, 3), (257, 1), (65, 65)])
def test_reset_flags_restart_only_the_flagged_envs(packed, rows, per_env):
    from gym_uav_collision_avoidance_amd.exploration import launch
    envs, x_init = rows // per_env, 0.625
    ex = _explore("ddpg", rows, seed=4, ou_sigma=0.5, ou_x_initial=x_init)
    obs = _obs(rows, seed=3)
    for _ in range(3):
        ex.act(obs)
    x0, n0, _ = _state(ex)
    assert (x0 != x_init).all() and (n0 == 3).all()
    rs = np.random.RandomState(rows)
    flagged = rs.rand(envs) < 0.5
    flagged[0] = True
    if envs > 1:
        flagged[-1] = False
    used = torch.zeros((rows, 2), dtype=torch.float64, device=DEV)
    if packed:                   # stride N = 3 bytes, bit 1 of agent 0's byte, every other bit of the three bytes set at random
        N = 3
        byte = rs.randint(0, 256, (envs, N)).astype(np.uint8)
        byte[:, 0] = (byte[:, 0] & ~np.uint8(2)) | (flagged.astype(np.uint8) << 1)
        flags = torch.from_numpy(byte).to(DEV)
        out = torch.empty((rows, 2), dtype=torch.float32, device=DEV)
        ex.actor._launch(obs, None, 0.0, _actor_lib.RAW, ex._raw, 2)
        rc = launch(ex._lib, stream(ex.device), kind=ex.kind, rows=rows, seed=ex.seed, raw=ex._raw.data_ptr(), raw_stride=2,
                    out=out.data_ptr(), out_stride=2, state=ex.state.data_ptr(), normals_out=used.data_ptr(),
                    reset_flags=flags.data_ptr(), reset_stride=N, reset_mask=2, rows_per_env=per_env,
                    ou_sigma=ex.ou_sigma, ou_theta=ex.ou_theta, ou_dt=ex.ou_dt, ou_x_initial=x_init)
        assert rc == _actor_lib.OK
    else:                        # stride 1, mask 1: bits other than bit 0 do not count
        byte = (flagged.astype(np.uint8) | (rs.randint(0, 128, envs).astype(np.uint8) << 1)).astype(np.uint8)
        out = ex.act(obs, reset=torch.from_numpy(byte).to(DEV), normals_out=used)
    row_flag = np.repeat(flagged, per_env)
    start = np.where(row_flag, x_init, x0)
    want = er.ou_step(start, used.cpu().numpy()[:, 0], ex.ou_sigma)
    x, n, _ = _state(ex)
    assert np.array_equal(x, want) and (n == 4).all()          # n is not reset
    cont = er.ou_step(x0, used.cpu().numpy()[:, 0], ex.ou_sigma)
    assert (x[row_flag] != cont[row_flag]).all() and np.array_equal(x[~row_flag], cont[~row_flag])
    det = ex.actor.act(obs).cpu().numpy().astype(np.float64)
    assert np.array_equal(out.cpu().numpy().view(np.int32), np.clip(det + x[:, None], -1, 1).astype(np.float32).view(np.int32))


# ---- 7. strided output, rejected calls --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ACTORS))
def test_strided_output_touches_only_its_cells_and_rejected_calls_nothing(name):
    from gym_uav_collision_avoidance_amd.exploration import launch
    for rows in ROWS:
        ex, twin = _explore(name, rows, seed=8), _explore(name, rows, seed=8)
        obs = _obs(rows, seed=rows)
        arena = torch.full((rows + 2, 6), float("nan"), device=DEV)
        got = ex.act(obs, out=arena[1:rows + 1, 2:4])
        assert got.data_ptr() == arena[1:rows + 1, 2:4].data_ptr()
        assert _same(arena[1:rows + 1, 2:4], twin.act(obs))
        mask = torch.ones_like(arena, dtype=torch.bool)
        mask[1:rows + 1, 2:4] = False
        assert bool(torch.isnan(arena[mask]).all()) and not bool(torch.isnan(arena[~mask]).any())
        before, state = arena.clone(), ex.state.clone()
        common = dict(kind=ex.kind, rows=rows, raw=ex._raw.data_ptr(), raw_stride=ex._cols, out=arena[1:, 2:].data_ptr(),
                      out_stride=6, state=ex.state.data_ptr())
        for wrong in (dict(out_stride=3), dict(rows=0), dict(random_prob=2.0), dict(out=arena.data_ptr() + 4),
                      dict(state=ex.state.data_ptr() + 8), dict(kind=5), dict(row_offset=-1)):
            assert launch(ex._lib, stream(ex.device), **dict(common, **wrong)) == _actor_lib.ERR_INVALID_ARG, wrong
        torch.cuda.synchronize()
        assert _same(torch.nan_to_num(arena, nan=5.0), torch.nan_to_num(before, nan=5.0)) and _same(ex.state, state)


# ---- 8. graph capture -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ACTORS))
def test_graph_replays_equal_eager_calls_across_the_warmup_boundary(name):
    rows = 257
    kw = dict(seed=21, warmup_steps=3, ou_sigma=0.3, random_prob=0.25)
    obs = _obs(rows, seed=2)
    _explore(name, rows, **kw).act(obs)                          # loads both kernels before the capture
    eager, graphed = _explore(name, rows, **kw), _explore(name, rows, **kw)
    want = [eager.act(obs).clone() for _ in range(5)]
    out = torch.zeros((rows, 2), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.act(obs, out=out)
    assert (_state(graphed)[1] == 0).all()                       # a capture runs nothing
    for k in range(5):
        g.replay()
        assert _same(out, want[k]), (name, k)
    assert _same(graphed.state, eager.state) and (_state(graphed)[1] == 5).all()
    assert not _same(want[2], want[3])
    # annealing reaches the captured launch through the device slot
    eager.set_random_prob(1.0)
    graphed.set_random_prob(1.0)
    g.replay()
    assert _same(out, eager.act(obs))
    sd = graphed.state_dict()
    fresh = _explore(name, rows, **kw).load_state_dict(sd)
    assert _same(fresh.state, graphed.state) and fresh.random_prob == 1.0 and _same(fresh.act(obs), eager.act(obs))


# ---- 9. learners ------------------------------------------------------------------------------------------------------
def _learner(kind, **kw):
    import learner_ref as lr
    from gym_uav_collision_avoidance_amd import learners
    cls = {"sac": learners.FusedSAC, "td3": learners.FusedTD3, "ddpg": learners.FusedDDPG}[kind]
    return lr.load_recipe(cls(device=DEV, **kw), kind).refresh()


def _batches(kind, rows, n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *shape: torch.rand(shape, generator=g, device=DEV) * 2 - 1
    out = []
    for _ in range(n):
        batch = (rnd(rows, 10), rnd(rows, 2), torch.randn(rows, generator=g, device=DEV), rnd(rows, 10),
                 (torch.rand(rows, generator=g, device=DEV) > 0.1).float())
        noise = tuple(torch.randn((rows, 2), generator=g, device=DEV) for _ in range({"sac": 2, "td3": 1, "ddpg": 0}[kind]))
        out.append((batch, noise or None))
    return out


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_select_action_with_exploration_follows_the_actor_steps(kind):
    agent = _learner(kind)
    live = agent.policy if kind == "sac" else agent.actor
    obs = torch.rand((5, 4, 10), generator=torch.Generator(device=DEV).manual_seed(9), device=DEV) * 2 - 1
    ex = agent.exploration(20, seed=6)
    assert ex.actor is agent._actor_h and ex.rows == 20
    if kind == "ddpg":
        assert ex.ou_sigma == agent.noise_std_dev
    if kind == "td3":
        assert ex.noise_std == 0.1
    seen = []
    for batch, noise in [(None, None)] + _batches(kind, 32, 3, seed=600):
        if batch is not None:
            agent.update_batch(*batch, noise=noise)
            if kind != "sac":
                assert agent._stale == (kind == "ddpg" or len(seen) != 2)
        got = agent.select_action(obs, explore=ex)
        if kind != "sac":
            assert agent._stale is False                        # the re-pack flag, as without `explore`
        assert got.shape == (5, 4, 2) and bool(torch.isfinite(got).all()) and float(got.abs().max()) <= 1.0
        raw = ex._raw.clone()                                   # what the exploration launch read: the live actor's heads
        assert float((raw - _heads(live, obs.reshape(20, 10))).abs().max()) <= 1e-5
        seen.append(raw)
    moved = [not torch.equal(a, b) for a, b in zip(seen, seen[1:])]
    assert moved == ([True, False, True] if kind == "td3" else [True] * 3)      # TD3's update 1 leaves the actor alone
    assert (_state(ex)[1] == 4).all()
    other = _learner(kind)
    with pytest.raises(ValueError, match="another actor"):
        other.select_action(obs, explore=ex)
    # without `explore` nothing changed
    assert torch.equal(agent.select_action(obs, evaluate=True), agent._actor_h.act(obs))
    other.close()
    agent.close()


@pytest.mark.parametrize("kind,packed", [("sac", False), ("td3", True), ("ddpg", False), ("ddpg", True)])
def test_closed_loop_writes_the_ring_and_restarts_ou_per_episode(kind, packed):
    from gym_uav_collision_avoidance_amd import UAVVectorEnv
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    E, N, T, x_init = 8, 4, 16, 0.5
    venv = UAVVectorEnv(E, num_agents=N, device=DEV, seed=2)
    mem = DeviceReplay(venv.env, horizon=32, packed_flags=packed)
    mem.begin(venv.reset())
    agent = _learner(kind)
    # sigma 0: the OU value decays from x_initial by a known factor per call, so it counts the calls since the restart
    ex = agent.exploration(mem, seed=5, warmup_steps=2, reset_on_episode=True, ou_sigma=0.0, ou_x_initial=x_init)
    assert ex.rows == E * N and ex.memory is mem
    want = np.full(E, x_init)
    restarts = 0
    for t in range(T):
        slot = mem.action_slot()
        slot.fill_(float("nan"))
        out = agent.select_action(mem.state, explore=ex, out=slot)
        assert out.data_ptr() == slot.data_ptr()
        a = mem.act[t % mem.L]
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) <= 1.0
        if t > 0:
            prev = (t - 1) % mem.L
            flag = ((mem.done[prev, :, 0] & 2) != 0) if packed else (mem.skip[prev] != 0)
            flag = flag.cpu().numpy()
            want = np.where(flag, x_init, want)
            restarts += int(flag.sum())
        if kind == "ddpg" and t >= 2:                           # warm-up calls leave x alone
            want = er.ou_step(want, 0.0, 0.0)
        if kind == "ddpg":
            assert np.array_equal(_state(ex)[0].reshape(E, N), np.repeat(want[:, None], N, axis=1)), t
        mem.step(polar=True, auto_reset="agent0_done", step_cap=4)
    assert restarts > 0 and (_state(ex)[1] == T).all()
    assert mem.count == T and bool((mem.act[:T] != 0).any(dim=-1).all())
    agent.close()
    venv.close()

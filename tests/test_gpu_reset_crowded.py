"""The reset accept / reject chain on CROWDED layouts, all three device implementations (csrc/uavx_multi_reset.hpp) against the
oracle's sequential loop: reset_envs_wave behind uavx_reset and behind the in-place auto-reset of a step workgroup (ballot and LDS
forms of lowest_clash, fixed-N templates, runtime N, bodies in trips), and stage_ahead (one lane per slot; incremental clash
bitmap on one wavefront, full re-test on several; attempts 0 and 1 pre-drawn, later ones on demand).

The cases are tests/reset_layouts.py CROWDED: boxes in which most envs need a third candidate for some slot and many a fifth, a
redraw regularly makes or frees a clash of a higher slot, bodies clash with learners, targets with their own starts.
tests/test_reset_layouts_host.py proves on the CPU that these events are present in every case, that no slot needs more than 512
candidates on any seed, world and episode index used here (so that no device loop runs long), and that the numpy restatement
they are counted on equals the oracle.  A wrong bit in the chain does not crash: it yields a legal layout from another stream
position, which only a bit-for-bit comparison with the sequential loop notices.

Compared as tests/test_gpu_ext.py does: state, bodies, levels, masks and counters bit for bit, observations and rewards within
that file's TOL."""
import numpy as np
import pytest

import reset_layouts as rl
import test_gpu_ext as ext
from golden_util import obs_err

pytestmark = pytest.mark.gpu
TOL, _np, _compare_state = ext.TOL, ext._np, ext._compare_state
NAMES = [c.name for c in rl.CROWDED]


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available()
    import gym_uav_collision_avoidance_amd as pkg
    return pkg


def _pair(amd, oracle_mod, case, E=None, env_offset=None):
    E = case.E if E is None else E
    off = case.env_offset if env_offset is None else env_offset
    env = amd.BatchedMultiUAVWorld2D(E, seed=case.seed, env_offset=off, **rl.env_kwargs(case))
    orc = oracle_mod.OracleMulti(num_envs=E, nthreads=8, **rl.env_kwargs(case))
    if case.levels:
        env.set_curriculum(case.levels, *case.window)
        orc.set_curriculum(case.levels, *case.window)
    return env, orc


def _same(env, orc, case, ctx, obs=None):
    if case.levels:
        np.testing.assert_array_equal(_np(env.env_levels()), orc.level, err_msg=f"{ctx} levels")
    _compare_state(env, orc, ctx)
    if obs is not None:
        assert obs_err(_np(obs), orc.observe()) <= TOL, ctx


def _step(env, orc, case, a, cap, seed, ctx, env_offset=None):
    import torch
    off = case.env_offset if env_offset is None else env_offset
    obs_g, rew_g, done_g, info = env.step_ex(torch.from_numpy(a).to(env.device), polar=True, auto_reset="agent0_done", step_cap=cap)
    obs_o, rew_o, done_o, rm_o, en_o, tr_o = orc.step_ex(a, action_mode=1, reset_policy=1, step_cap=cap, seed=seed, env_offset=off,
                                                         with_end=True)
    np.testing.assert_array_equal(_np(info["reset_mask"]).astype(np.uint8), rm_o, err_msg=ctx)
    np.testing.assert_array_equal(_np(info["ended"]).astype(np.uint8), en_o, err_msg=ctx)
    np.testing.assert_array_equal(_np(info["truncated"]).astype(np.uint8), tr_o, err_msg=ctx)
    np.testing.assert_array_equal(_np(done_g).astype(np.uint8), done_o, err_msg=ctx)
    _same(env, orc, case, ctx)
    assert obs_err(_np(obs_g), obs_o) <= TOL and float(np.abs(_np(rew_g) - rew_o).max()) <= TOL, ctx
    return int(rm_o.sum()), (obs_g, rew_g, done_g, info["reset_mask"])


def _scattered_mask(E, L, rng):
    """Envs picked so that `go` differs between the envs of one wavefront and between the wavefronts of one workgroup: random
    ones, runs of selected and of unselected envs, and every wavefront-sized block handled differently from its neighbour."""
    per_wave = max(1, 64 // L)
    mask = rng.random(E) < 0.4
    block = np.arange(E) // per_wave
    mask[block % 5 == 0] = True          # a whole wavefront resets ...
    mask[block % 5 == 1] = False         # ... the next one sits out
    mask[block % 5 == 2] = (np.arange(E) % 2 == 0)[block % 5 == 2]
    return mask


@pytest.mark.parametrize("name", NAMES)
def test_explicit_reset(amd, oracle_mod, name):
    """uavx_reset (reset_envs_wave): every env, then a scattered mask, then every env under another seed."""
    import torch
    case = rl.BY_NAME[name]
    env, orc = _pair(amd, oracle_mod, case)
    obs = env.reset(); orc.reset_philox(case.seed, env_offset=case.env_offset)
    _same(env, orc, case, f"case {name}: reset", obs)
    mask = _scattered_mask(case.E, case.L, np.random.default_rng(case.seed))
    obs = env.reset(mask=torch.from_numpy(mask).to(env.device)); orc.reset_philox(case.seed, mask=mask, env_offset=case.env_offset)
    _same(env, orc, case, f"case {name}: masked reset", obs)
    obs = env.reset(seed=case.seed2); orc.reset_philox(case.seed2, env_offset=case.env_offset)
    _same(env, orc, case, f"case {name}: reset under another seed", obs)
    assert (orc.counters[:, 3] == 2 + mask).all()
    env.close()


IN_PLACE = ([(n, None, None) for n in NAMES if n not in ("13", "24")] + [("8", "UAVX_TILES", 2)] +
            [(n, "UAVX_GW", w) for n in ("13", "24") for w in (1, 2, 3, 4)])


@pytest.mark.parametrize("name,switch,value", IN_PLACE)
def test_auto_reset_in_place(amd, oracle_mod, monkeypatch, name, switch, value):
    """No layouts drawn ahead: every second call re-initialises every env inside its step workgroup (step cap 1).  The cases
    cover the fixed-N templates (2, 4, 5, 8 learners, the 8-UAV kernel also with two tiles per workgroup), runtime N, and the
    extension kernels; 13 and 24 learners run on 1, 2, 3 and 4 wavefronts per workgroup -- the ballot and the LDS form of
    lowest_clash on identical input."""
    case = rl.BY_NAME[name]
    if switch:
        monkeypatch.setenv(switch, str(value))
    env, orc = _pair(amd, oracle_mod, case)
    env.set_prefetch(0)
    env.reset(); orc.reset_philox(case.seed, env_offset=case.env_offset)
    rng = np.random.default_rng(case.seed)
    resets = 0
    for t in range(12):
        a = rng.uniform(-1, 1, size=(case.E, case.L, 2)).astype(np.float32)
        resets += _step(env, orc, case, a, 1, case.seed, f"case {name} {switch}={value} step {t}")[0]
    assert resets == 6 * case.E
    env.close()


@pytest.mark.parametrize("behind", [0, 1])
@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_auto_reset_staged(amd, oracle_mod, monkeypatch, name, cap, behind):
    """Staging workgroups in every launch (stage_ahead), in front of and behind the env-workgroups, episodes of one and two
    steps: both parked layouts of an env are consumed and drawn again several times.  The seed changes at one step and the world
    at a later one (set_config to another crowded box; with a curriculum the level window moves): layouts parked for the old
    seed or the old world must not be used."""
    case = rl.BY_NAME[name]
    monkeypatch.setenv("UAVX_STAGE_BEHIND", str(behind))
    env, orc = _pair(amd, oracle_mod, case)
    env.set_prefetch(1)
    env.reset(); orc.reset_philox(case.seed, env_offset=case.env_offset)
    rng = np.random.default_rng(case.seed + cap)
    seed, resets = case.seed, 0
    for t in range(16):
        if t == 6:
            seed = case.seed2
            env.seed = seed
        if t == 11:
            if case.levels:
                env.set_level_window(*case.window2); orc.set_level_window(*case.window2)
            else:
                env.set_config(x_size=case.box2[0], y_size=case.box2[1]); orc.set_config(x_size=case.box2[0], y_size=case.box2[1])
        a = rng.uniform(-1, 1, size=(case.E, case.L, 2)).astype(np.float32)
        resets += _step(env, orc, case, a, cap, seed, f"case {name} cap {cap} behind {behind} step {t}")[0]
    assert resets >= (16 // (cap + 1) - 1) * case.E
    assert int(orc.counters[:, 3].max()) <= rl.EPISODES - 1      # (the layout parked beyond it is the last index the host test covers)
    env.close()


@pytest.mark.parametrize("name", ["8", "8+16", "24"])
def test_paths_agree(amd, name):
    """A PROPERTY test, GPU against GPU: drawing in place, staging in every launch and staging at a slow cadence give the same
    run bit for bit.  It says nothing the tests above do not say, but it points at the one path that is off when they fail."""
    import torch
    case = rl.BY_NAME[name]
    runs = []
    for prefetch in (0, 1, 16):
        env = amd.BatchedMultiUAVWorld2D(case.E, seed=case.seed, env_offset=case.env_offset, **rl.env_kwargs(case))
        env.set_prefetch(prefetch)
        out = [env.reset().clone()]
        g = torch.Generator(device="cpu").manual_seed(case.seed)
        for t in range(10):
            a = (torch.rand((case.E, case.L, 2), generator=g) * 2 - 1).to(env.device)
            o, r, d, info = env.step_ex(a, polar=True, auto_reset="agent0_done", step_cap=1)
            out += [o.clone(), r.clone(), d.clone(), info["reset_mask"].clone()]
        st = env.get_state()
        out += [st[k] for k in ("loc", "vel", "tgt", "init_d", "prev_d", "flags", "counters")]
        if case.B:
            out.append(env.get_bodies())
        runs.append(out)
        env.close()
    for prefetch, run in zip((1, 16), runs[1:]):
        for k, (x, y) in enumerate(zip(runs[0], run)):
            same = torch.equal(x, y)
            assert same, f"case {name}: prefetch {prefetch} differs from in-place drawing at item {k}"


@pytest.mark.parametrize("name", ["5", "8+16"])
def test_large_env_offset_shard_cut(amd, oracle_mod, name):
    """Global env ids past 2^40 (bits 32-47 travel in Philox counter word 1 beside the slot): the batch equals the oracle, and
    its two halves, created at their own offsets, equal the batch."""
    import torch
    case = rl.BY_NAME[name]
    assert case.env_offset == rl.BIG_OFFSET
    E = case.E - case.E % 2
    half = E // 2
    env, orc = _pair(amd, oracle_mod, case, E=E)
    parts = [amd.BatchedMultiUAVWorld2D(half, seed=case.seed, env_offset=case.env_offset + k * half, **rl.env_kwargs(case)) for k in (0, 1)]
    obs = env.reset(); orc.reset_philox(case.seed, env_offset=case.env_offset)
    _same(env, orc, case, f"case {name}: reset", obs)
    po = [p.reset() for p in parts]
    assert torch.equal(obs, torch.cat(po, dim=0))
    rng = np.random.default_rng(3)
    for t in range(6):
        a = rng.uniform(-1, 1, size=(E, case.L, 2)).astype(np.float32)
        _, whole = _step(env, orc, case, a, 1, case.seed, f"case {name} step {t}")
        cut = [p.step_ex(torch.from_numpy(a[k * half:(k + 1) * half]).to(p.device), polar=True, auto_reset="agent0_done", step_cap=1)
               for k, p in enumerate(parts)]
        for i in range(3):
            assert torch.equal(whole[i], torch.cat([c[i] for c in cut], dim=0)), f"case {name} step {t} output {i}"
        assert torch.equal(whole[3], torch.cat([c[3]["reset_mask"] for c in cut], dim=0))
    sw, sp = env.get_state(), [p.get_state() for p in parts]
    for k in ("loc", "tgt", "flags", "counters"):
        assert torch.equal(sw[k], torch.cat([s[k] for s in sp], dim=0)), k
    if case.B:
        assert torch.equal(env.get_bodies(), torch.cat([p.get_bodies() for p in parts], dim=0))
    env.close()
    for p in parts:
        p.close()


def test_large_env_offset_single_uav_world(amd, oracle_mod):
    """BatchedUAVWorld2D at the same offset: reset and the auto-reset of step_ex (PhiloxDraws packs the env id on its own)."""
    E, seed = 700, 41
    env = amd.BatchedUAVWorld2D(E, x_size=12.0, y_size=10.0, seed=seed, env_offset=rl.BIG_OFFSET)
    orc = oracle_mod.OracleSingle(num_envs=E, x_size=12.0, y_size=10.0, nthreads=8)
    env.reset(); orc.reset_philox(seed, env_offset=rl.BIG_OFFSET)
    rng = np.random.default_rng(2)
    resets = 0
    for t in range(10):
        st = env.get_state()
        np.testing.assert_array_equal(_np(st["loc"]), orc.loc.astype(np.float32), err_msg=f"step {t}")
        np.testing.assert_array_equal(_np(st["tgt"]), orc.tgt.astype(np.float32), err_msg=f"step {t}")
        np.testing.assert_array_equal(_np(st["counters"])[:, 1], orc.episode, err_msg=f"step {t}")
        act = rng.uniform(-1, 1, size=(E, 2)).astype(np.float32)
        og, rg, dg, info = env.step_ex(act, polar=True, auto_reset=True, step_cap=1)
        oo, ro, do, io, rm = orc.step_ex(act, polar=True, auto_reset=True, step_cap=1, seed=seed, env_offset=rl.BIG_OFFSET)
        np.testing.assert_array_equal(_np(info["reset_mask"]).astype(np.uint8), rm, err_msg=f"step {t}")
        np.testing.assert_array_equal(_np(dg).astype(np.uint8), do, err_msg=f"step {t}")
        assert obs_err(_np(og), oo, (1, 3)) <= TOL, t
        resets += int(rm.sum())
    assert resets == 5 * E
    # the same envs in a batch that starts 300 envs earlier: the id, not the position in the batch, addresses the stream
    other = amd.BatchedUAVWorld2D(E, x_size=12.0, y_size=10.0, seed=seed, env_offset=rl.BIG_OFFSET - 300)
    a, b = amd.BatchedUAVWorld2D(E, x_size=12.0, y_size=10.0, seed=seed, env_offset=rl.BIG_OFFSET), other
    a.reset(); b.reset()
    sa, sb = a.get_state(), b.get_state()
    for k in ("loc", "tgt"):
        assert bool((sa[k][:E - 300] == sb[k][300:]).all()), k
    for h in (env, a, b):
        h.close()

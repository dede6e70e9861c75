"""Near ties and the sensing limit of the 6-64 UAV neighbour key scan (scan_neighbours, N > 5 and the 8-UAV specialisation) on
the crafted layouts of tests/key_scan_layouts.py, against the CPU oracle.  Nothing is masked; 1e-5 on observations and rewards
(DESIGN section 6), everything else bit for bit.  tests/test_key_scan_layouts_host.py shows on the CPU what these batches hold:
every boundary of the near-tie predicate, wavefronts with exactly 0, 1, 6, 7 and all lanes tied, tied lanes at lane 0, at the
last active lane, in the later wavefronts of a workgroup and in envs that straddle two wavefronts.

* observe() and one step() at n = 6, 7, 8 (one and two tiles), 10, 13, 24, 64 and four sensing ranges;
* launch-shape independence: the same batch under 1-4 wavefronts per workgroup is bit-identical (the same tied egos move
  between wavefronts and across the 6 / 7 switch between the per-lane and the whole-wavefront rescan);
* step() == step_k == step_ex bit for bit;
* scripted bodies and levels (the kernels with bodies in the neighbour rows): learner-body and body-body ties, envs of one
  wavefront with different sensing ranges and parked slots."""
import numpy as np
import pytest

import key_scan_layouts as kl
import neighbour_layouts as nl
from golden_util import obs_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
WORLD = dict(collider_radius=0.2, **kl.WORLD)     # small colliders: the crafted neighbours are no collisions
CASES = [(n, d, 0) for n in kl.AGENTS for d in kl.SENSE] + [(8, d, 2) for d in kl.SENSE]   # (agents, d_sense, UAVX_TILES or 0)
_cache = {}


def _batch(n, d, **kw):
    key = (n, d, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = kl.make_batch(n, d, **kw)
    return _cache[key]


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import gym_uav_collision_avoidance_amd as pkg
    return pkg


def _np(t):
    return t.detach().cpu().numpy()


def _device(amd, b, n, d_sense, vel, seed=11):
    """A device batch holding the crafted positions, velocities `vel` and the natural prev_distance (targets: the reset's)."""
    E = b["loc"].shape[0]
    env = amd.BatchedMultiUAVWorld2D(E, num_agents=n, d_sense=d_sense, seed=seed, **WORLD)
    env.reset()
    tgt = _np(env.get_state()["tgt"])
    env.set_state(loc=b["loc"], vel=vel, prev_d=nl.natural_prev_d(b["loc"], tgt))
    return env


def _pair(amd, oracle_mod, b, n, d_sense, vel, seed=11):
    E = b["loc"].shape[0]
    env = _device(amd, b, n, d_sense, vel, seed)
    orc = oracle_mod.OracleMulti(num_envs=E, num_agents=n, d_sense=d_sense, nthreads=8, **WORLD)
    orc.reset_philox(seed)
    tgt = _np(env.get_state()["tgt"])
    np.testing.assert_array_equal(orc.tgt.astype(np.float32), tgt)
    orc.set_state(loc=b["loc"], vel=vel, prev_d=nl.natural_prev_d(b["loc"], tgt))
    return env, orc


def _check_state(env, orc, ctx):
    st, ref = {k: _np(v) for k, v in env.get_state().items()}, orc.get_state()
    for k in ("flags", "loc", "vel", "prev_d"):
        np.testing.assert_array_equal(st[k], ref[k], err_msg=f"{ctx} {k}")
    np.testing.assert_array_equal(st["counters"][:, :3], ref["counters"][:, :3], err_msg=ctx + " counters")


def _worst(b, g, o):
    """Where the observations differ most: (error, env, agent, column, class of that ego or '-', wavefront, lane)."""
    err = np.abs(np.asarray(g, np.float64) - o)
    err[..., [1, 3, 5, 6, 8, 9]] = np.minimum(err[..., [1, 3, 5, 6, 8, 9]], 2.0 - err[..., [1, 3, 5, 6, 8, 9]])
    e, i, c = np.unravel_index(np.argmax(err), err.shape)
    cls = [k for ee, ii, k in zip(b["ego_env"], b["ego_i"], b["ego_cls"]) if ee == e and ii == i] or ["-"]
    wave, lane = kl.lane_table(b["loc"].shape[0], b["n"], b["W"], b["epw"])
    return float(err[e, i, c]), int(e), int(i), int(c), cls[0], int(wave[e, i]), int(lane[e, i])


@pytest.mark.parametrize("n,d_sense,tiles", CASES)
def test_key_scan_crafted_observe_and_step(amd, oracle_mod, monkeypatch, n, d_sense, tiles):
    """Every class and wavefront kind, unmasked: observe() with distinct headings (a wrong neighbour moves a heading column by
    >= 1.2 / n), then one step() from zero velocity with zero commands (the layout stays where it was built)."""
    if tiles:
        monkeypatch.setenv("UAVX_TILES", str(tiles))
    elif n == 8:
        monkeypatch.setenv("UAVX_TILES", "1")
    b = _batch(n, d_sense)
    E = b["loc"].shape[0]
    env, orc = _pair(amd, oracle_mod, b, n, d_sense, b["vel"])
    g, o = _np(env.observe()), orc.observe()
    assert obs_err(g, o) <= TOL, f"observe n={n} d_sense={d_sense}: {_worst(b, g, o)}"
    env.close()
    env, orc = _pair(amd, oracle_mod, b, n, d_sense, np.zeros_like(b["vel"]))
    act = np.zeros((E, n, 2), np.float32)
    og, rg, dg, _ = env.step(act)
    oo, ro, do = orc.step(act)
    ctx = f"step n={n} d_sense={d_sense}"
    np.testing.assert_array_equal(_np(dg).astype(np.uint8), do, err_msg=ctx)
    _check_state(env, orc, ctx)
    np.testing.assert_array_equal(orc.loc.astype(np.float32), b["loc"], err_msg=ctx + " layout moved")
    assert obs_err(_np(og), oo) <= TOL, f"{ctx}: {_worst(b, _np(og), oo)}"
    assert float(np.abs(_np(rg) - ro).max()) <= TOL, ctx
    env.close()


@pytest.mark.parametrize("n,d_sense", [(n, d) for n in (6, 7, 10, 24) for d in kl.SENSE])
def test_key_scan_launch_shape_independence(amd, monkeypatch, n, d_sense):
    """The same crafted batch under UAVX_GW = 1, 2, 3, 4 wavefronts per workgroup: observations, rewards, dones and state are
    bit-identical.  The host model gives another set of tied lanes per wavefront for every W (checked here), so the same tied
    egos are resolved by the per-lane rescan under one W and by the whole-wavefront scan under another."""
    b = _batch(n, d_sense)
    E = b["loc"].shape[0]
    counts = [tuple(kl.tied_lanes_per_wave(b["loc"], n, d_sense, W).tolist()) for W in (1, 2, 3, 4)]
    assert len(set(counts)) == 4
    assert all(any(1 <= c <= 6 for c in cs) and any(c >= 7 for c in cs) for cs in counts)
    ref = None
    for W in (1, 2, 3, 4):
        monkeypatch.setenv("UAVX_GW", str(W))
        env = _device(amd, b, n, d_sense, b["vel"])
        obs0 = _np(env.observe()).copy()
        env.close()
        env = _device(amd, b, n, d_sense, np.zeros_like(b["vel"]))
        o, r, d, _ = env.step(np.zeros((E, n, 2), np.float32))
        got = dict(observe=obs0, obs=_np(o).copy(), rew=_np(r).copy(), done=_np(d).copy(),
                   **{"state " + k: _np(v) for k, v in env.get_state().items()})
        env.close()
        if ref is None:
            ref = got
        for k in ref:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"n={n} d_sense={d_sense} UAVX_GW={W} {k}")


@pytest.mark.parametrize("n,d_sense,tiles", [(n, d, 0) for n in (6, 13, 64) for d in kl.SENSE]
                         + [(8, d, t) for d in kl.SENSE for t in (1, 2)])
def test_key_scan_variants_agree_bit_for_bit(amd, monkeypatch, n, d_sense, tiles):
    """K step() calls == step_k(K, tape_out=True) for K = 1 and 3 == K step_ex() calls with defaults, bit for bit on the crafted
    layouts (step_kernel, step_k_kernel and step_ex_kernel each inline the scan)."""
    import torch
    if tiles:
        monkeypatch.setenv("UAVX_TILES", str(tiles))
    b = _batch(n, d_sense)
    E = b["loc"].shape[0]
    zero = np.zeros_like(b["vel"])
    for K in (1, 3):
        envs = [_device(amd, b, n, d_sense, zero) for _ in range(3)]
        tape = torch.zeros((K, E, n, 2), dtype=torch.float32, device=envs[0].device)
        ref = []
        for k in range(K):
            o, r, d, _ = envs[0].step(tape[k])
            ref.append((_np(o).copy(), _np(r).copy(), _np(d).copy()))
        ko, kr, kd, _ = envs[1].step_k(tape, tape_out=True)
        ko, kr, kd = _np(ko), _np(kr), _np(kd)
        for k in range(K):
            eo, er, ed, _ = envs[2].step_ex(tape[k])
            ctx = f"n={n} d_sense={d_sense} K={K} step {k}"
            for got in ((ko[k], kr[k], kd[k]), (_np(eo), _np(er), _np(ed))):
                np.testing.assert_array_equal(got[0], ref[k][0], err_msg=ctx + " obs")
                np.testing.assert_array_equal(got[1], ref[k][1], err_msg=ctx + " rew")
                np.testing.assert_array_equal(got[2].astype(bool), ref[k][2].astype(bool), err_msg=ctx + " done")
        s = [{k: _np(v) for k, v in e.get_state().items()} for e in envs]
        for key in s[0]:
            np.testing.assert_array_equal(s[1][key], s[0][key], err_msg=f"step_k state {key}")
            np.testing.assert_array_equal(s[2][key], s[0][key], err_msg=f"step_ex state {key}")
        np.testing.assert_array_equal(s[0]["loc"], b["loc"], err_msg="layout moved")
        for e in envs:
            e.close()


# ---------------------------------------------------------------------------------------------------------------------------
# scripted bodies and levels
LEVELS = [dict(d_sense=9.0, n_active=6, b_active=3, collider_radius=0.2, **kl.WORLD),
          dict(d_sense=7.3, n_active=5, b_active=2, collider_radius=0.2, **kl.WORLD)]


def _levels_batch():
    """6 learners + 3 bodies, envs alternating between the two LEVELS: even envs from the batch crafted for level 0, odd envs from
    the one crafted for level 1 (a parked learner and a switched-off body at +inf), the tied egos at their own env's limit."""
    if "levels" not in _cache:
        tied = ("Ftie-a", "Ftie-b", "Ftie-c", "B", "C")
        b0 = kl.make_batch(6, 9.0, bodies=3, tied=tied)
        b1 = kl.make_batch(6, 7.3, bodies=3, tied=tied, n_active=5, b_active=2)
        E = b0["loc"].shape[0]
        assert b1["loc"].shape[0] == E
        odd = np.arange(E) % 2 == 1
        b = dict(b0)
        b["loc"] = np.where(odd[:, None, None], b1["loc"], b0["loc"])
        b["d_env"] = np.where(odd, 7.3, 9.0)
        for k in ("ego_env", "ego_i", "ego_cls", "ego_wave", "ego_lane"):
            b[k] = np.concatenate([b0[k][~odd[b0["ego_env"]]], b1[k][odd[b1["ego_env"]]]])
        _cache["levels"] = b
    return _cache["levels"]


def _ext_pair(amd, oracle_mod, b, L, B, d_sense, vel, levels=None):
    E = b["loc"].shape[0]
    kw = dict(num_agents=L, num_bodies=B, d_sense=d_sense, body_speed=0.0, body_period=128, body_seed=5, **WORLD)
    env = amd.BatchedMultiUAVWorld2D(E, seed=13, **kw)
    orc = oracle_mod.OracleMulti(num_envs=E, nthreads=8, **kw)
    if levels:
        assign = (np.arange(E) % 2).astype(np.uint8)
        env.set_curriculum(levels); orc.set_curriculum(levels)
        env.set_env_levels(assign); orc.set_env_levels(assign)
    env.reset()
    orc.reset_philox(13)
    if levels:
        np.testing.assert_array_equal(_np(env.env_levels()), assign)
    rec = _np(env.get_bodies()).copy()
    np.testing.assert_array_equal(np.isfinite(rec[..., 0]), np.isfinite(orc.body[..., 0]))
    on = np.isfinite(b["loc"][:, L:, 0])
    np.testing.assert_array_equal(on, np.isfinite(rec[..., 0]))          # the level's switched-off bodies are the batch's
    still = np.zeros_like(rec)
    still[..., :2] = b["loc"][:, L:]
    still[..., 4] = b["heading"][:, L:].astype(np.float32)
    rec = np.where(on[..., None], still, rec)                              # held still: zero displacement, no steps left
    env.set_bodies(rec)
    orc.body[...] = rec
    tgt = _np(env.get_state()["tgt"])
    np.testing.assert_array_equal(orc.tgt.astype(np.float32), tgt)
    loc = b["loc"][:, :L]
    parked = ~np.isfinite(loc[..., 0])
    np.testing.assert_array_equal(parked, (_np(env.get_state()["flags"]) & 32) != 0)
    prev = np.where(parked, _np(env.get_state()["prev_d"]), nl.natural_prev_d(np.where(parked[..., None], 0, loc), tgt))
    env.set_state(loc=loc, vel=vel, prev_d=prev)
    orc.set_state(loc=loc, vel=vel, prev_d=prev)
    return env, orc


def _ext_check(amd, oracle_mod, b, L, B, d_sense, levels=None):
    E = b["loc"].shape[0]
    env, orc = _ext_pair(amd, oracle_mod, b, L, B, d_sense, b["vel"], levels)
    g, o = _np(env.observe()), orc.observe()
    assert obs_err(g, o) <= TOL, f"observe {L}+{B}: {_worst(b, g, o)}"
    env.close()
    env, orc = _ext_pair(amd, oracle_mod, b, L, B, d_sense, np.zeros_like(b["vel"]), levels)
    act = np.zeros((E, L, 2), np.float32)
    og, rg, dg, _ = env.step(act)
    oo, ro, do = orc.step(act)
    ctx = f"step {L}+{B} d_sense={d_sense}"
    np.testing.assert_array_equal(_np(dg).astype(np.uint8), do, err_msg=ctx)
    _check_state(env, orc, ctx)
    np.testing.assert_array_equal(_np(env.get_bodies()), orc.body, err_msg=ctx + " bodies")
    np.testing.assert_array_equal(orc.loc.astype(np.float32), b["loc"][:, :L], err_msg=ctx + " layout moved")
    np.testing.assert_array_equal(orc.body[..., :2], np.where(np.isfinite(b["loc"][:, L:]), b["loc"][:, L:], orc.body[..., :2]),
                                  err_msg=ctx + " bodies moved")
    assert obs_err(_np(og), oo) <= TOL, f"{ctx}: {_worst(b, _np(og), oo)}"
    assert float(np.abs(_np(rg) - ro).max()) <= TOL, ctx
    env.close()


@pytest.mark.parametrize("L,B,d_sense", [(L, B, d) for L, B in ((6, 3), (8, 16)) for d in kl.SENSE])
def test_key_scan_with_scripted_bodies(amd, oracle_mod, L, B, d_sense):
    """Bodies in the neighbour rows (the `body` visits of the runtime-N scan and the rescans over L + B slots), held still.  The
    winners of half the egos are taken from the body slots: learner-body and body-body ties; a body has the higher slot, so a
    learner wins an equal root.  The oracle's extension part restates this build's own definition of bodies and levels (DESIGN
    section 3), not the reference: what is under test here is the (distance, slot) order over learners and bodies."""
    b = _batch(L, d_sense, bodies=B)
    tj, _ = kl.truth(b["loc"], b["sq_sense"])
    tie = kl.near_tie(b["loc"], b["sq_sense"])[:, :L]
    w = tj[:, :L][tie]                                                   # winners of the tied lanes: both kinds of pair occur
    assert ((w[:, 0] >= L) & (w[:, 1] >= L)).any() and ((w[:, 0] >= 0) & (w[:, 0] < L) & (w[:, 1] >= L)).any()
    cnt = kl.check_plan(b)
    assert {0, 1, 6, 7} <= set(cnt.tolist())
    _ext_check(amd, oracle_mod, b, L, B, d_sense)


def test_key_scan_with_levels_in_one_wavefront(amd, oracle_mod):
    """Two levels alternating from env to env (d_sense 9.0 with all 6 + 3 slots, 7.3 with a parked learner and a switched-off
    body at +inf): a tied ego at ITS env's limit in a wavefront with 1-6 tied lanes is rescanned by the whole wavefront, which
    must use the tied lane's limit, not its own.  Judged against the oracle with the same bodies and levels (the oracle's
    extension part restates this build's own definition, DESIGN section 3: the (distance, slot) order is under test)."""
    b = _levels_batch()
    E = b["loc"].shape[0]
    cnt = kl.tied_lanes_per_wave(b["loc"], 6, b["d_env"], 1, b["epw"])
    sq_env = np.array([nl.sq_limit_lt(d) for d in b["d_env"]], np.float32)
    tie = kl.near_tie(b["loc"], sq_env)[:, :6]
    at_limit = [(e, i) for e, i, c in zip(b["ego_env"], b["ego_i"], b["ego_cls"])
                if c.startswith("Ftie") and tie[e, i] and 1 <= cnt[e // b["epw"]] <= 6]
    assert len({e % 2 for e, _ in at_limit}) == 2 and len(at_limit) >= 8   # egos at either level's limit on the per-lane path
    for e, i in at_limit[:8]:                                            # ... whose class holds at the env's OWN limit only
        other = nl.sq_limit_lt(b["d_env"][(e + 1) % E])
        assert kl.classify(b["loc"][e], i, sq_env[e]) & {"Ftie-a", "Ftie-b", "Ftie-c"}
        assert not kl.classify(b["loc"][e], i, other) & {"Ftie-a", "Ftie-b", "Ftie-c"}
    _ext_check(amd, oracle_mod, b, 6, 3, 9.0, LEVELS)

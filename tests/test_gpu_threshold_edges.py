"""Every comparison of the step kernels that ends an episode or sets the -2 / +10 rewards, at one float step below, on and above
its limit, on the crafted batches of tests/threshold_layouts.py, against the CPU oracle.  tests/test_threshold_layouts_host.py
proves on the CPU that every member sits exactly where its tag says, that the oracle's decision flips between the two members a
class names, that the two sides' rewards differ by >= 0.5 where the decision shows there, and that the egos sit in wavefronts of
every exit of both neighbour scans; tests/golden/live_thresholds.npz pins the oracle to the reference on the same states.

Compared bit for bit: done, flags, positions, velocities, prev_distance, the first three counters.  Within 1e-5 (DESIGN
section 6): observations (angles on the circle) and rewards.  Nothing is masked.  Every test prints its worst observation and
reward error.

* step(), two steps (the second carries "a hard collision is counted once"), at n = 1, 2, 3, 4, 5, 7, 8 (one and two tiles), 13,
  24, float32 and float64 commands (separate template instances), evaluate 0 and 1 in the worlds with box members;
* step_k(K = 2, tape_out) and step_ex() at n = 4, 8, 13: each against the oracle, and bit for bit against step();
* step_ex with auto-reset: exactly the envs whose agent 0 finished or left the box are re-initialised by the next call, and with a
  step cap of 2 every other env ends in the second call;
* launch-shape independence at n = 7 and 24 under 1-4 wavefronts per workgroup;
* scripted bodies and levels (4 + 4 and 8 + 16): a body as the neighbour at the limit, two levels in one wavefront;
* float64-position mode at n = 3: the Python-float comparands, one float64 step either side;
* the single-UAV world: goal (+1000) and the four sides of the box, step() and step_ex, float32 and float64 commands, the state
  a reset leaves (float32 velocity) and a later one."""
import numpy as np
import pytest

import threshold_layouts as tl
from golden_util import obs_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
F32 = np.float32
STEP_CASES = [(n, c, 0) for n in (1, 2, 3, 4, 5, 7, 13, 24) for c in ("f32", "f64")] + \
             [(8, c, t) for c in ("f32", "f64") for t in (1, 2)]


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import gym_uav_collision_avoidance_amd as pkg
    return pkg


def _np(t):
    return t.detach().cpu().numpy()


def _commands(b):
    return b["act32"] if b["commands"] == "f32" else b["act"]


def _device(amd, b, seed=11):
    E, n = b["loc"].shape[:2]
    env = amd.BatchedMultiUAVWorld2D(E, num_agents=n, seed=seed, **tl.world_kwargs(b["world"]))
    env.reset()
    env.set_state(loc=b["loc"], vel=b["vel"], tgt=b["tgt"], init_d=b["init_d"], prev_d=b["prev_d"])
    return env


def _where(b, bad):
    """The first few differing (env, agent) named by class, member, wavefront and lane."""
    bad = np.asarray(bad)
    if bad.ndim == 1:
        return "; ".join(tl.describe(b, int(e)) for e in np.flatnonzero(bad)[:4])
    while bad.ndim > 2:
        bad = bad.any(-1)
    return "; ".join(tl.describe(b, int(e), int(i)) for e, i in zip(*np.nonzero(bad)))[:900]


def _same(b, got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    bad = got != ref
    assert not bad.any(), f"{what}: {_where(b, bad)}"


def _check(b, env, orc, out_g, out_o, ctx):
    """Device outputs and state against the oracle's; returns (worst observation error, worst reward error)."""
    (og, rg, dg), (oo, ro, do) = out_g, out_o
    _same(b, _np(dg).astype(np.uint8), do, ctx + " done")
    st, ref = {k: _np(v) for k, v in env.get_state().items()}, orc.get_state()
    for k in ("flags", "loc", "prev_d"):
        _same(b, st[k], ref[k], f"{ctx} {k}")
    _same(b, st["vel"].view(np.uint64), ref["vel"].view(np.uint64), ctx + " vel (float64 bits)")
    _same(b, (st["counters"][:, :3] != ref["counters"][:, :3].astype(np.int32)).any(-1), False, ctx + " counters")
    err = np.abs(_np(og).astype(np.float64) - oo)
    cols = [1, 3, 5, 6, 8, 9]
    err[..., cols] = np.minimum(np.mod(err[..., cols], 2.0), 2.0 - np.mod(err[..., cols], 2.0))
    assert obs_err(_np(og), oo) <= TOL, f"{ctx} obs {err.max():.3g}: {_where(b, err > TOL)}"
    rerr = np.abs(_np(rg).astype(np.float64) - ro)
    assert rerr.max() <= TOL, f"{ctx} reward {rerr.max():.3g}: {_where(b, rerr > TOL)}"
    return float(err.max()), float(rerr.max())


def _worlds(n):
    return [w for w in tl.WORLDS if tl.classes_of(n, w)]


@pytest.mark.parametrize("n,commands,tiles", STEP_CASES)
def test_step_at_every_threshold(amd, oracle_mod, monkeypatch, n, commands, tiles):
    if n == 8:
        monkeypatch.setenv("UAVX_TILES", str(tiles))
    worst = [0.0, 0.0]
    for world in _worlds(n):
        b = tl.make_threshold_batch(n, world, commands)
        for evaluate in (False, True) if "O" in tl.classes_of(n, world) else (False,):
            env, orc = _device(amd, b), tl.oracle_for(oracle_mod, b)
            for t in (1, 2):
                og, rg, dg, _ = env.step(_commands(b), evaluate=evaluate)
                out_o = orc.step(b["act"], evaluate=evaluate)
                e = _check(b, env, orc, (og, rg, dg), out_o, f"step {t} n={n} {world} {commands} evaluate={evaluate}")
                worst = [max(worst[0], e[0]), max(worst[1], e[1])]
            env.close()
    print(f"step n={n} {commands} tiles={tiles}: worst obs error {worst[0]:.3g}, worst reward error {worst[1]:.3g}")


def _check_outputs(b, out_g, out_o, ctx):
    """Outputs alone (no state) against the oracle's: done bit for bit, observations and rewards within TOL."""
    (og, rg, dg), (oo, ro, do) = out_g, out_o
    _same(b, np.asarray(dg).astype(np.uint8), do, ctx + " done")
    err = np.abs(np.asarray(og, np.float64) - oo)
    cols = [1, 3, 5, 6, 8, 9]
    err[..., cols] = np.minimum(np.mod(err[..., cols], 2.0), 2.0 - np.mod(err[..., cols], 2.0))
    assert err.max() <= TOL, f"{ctx} obs {err.max():.3g}: {_where(b, err > TOL)}"
    rerr = np.abs(np.asarray(rg, np.float64) - ro)
    assert rerr.max() <= TOL, f"{ctx} reward {rerr.max():.3g}: {_where(b, rerr > TOL)}"
    return float(err.max()), float(rerr.max())


@pytest.mark.parametrize("n,commands", [(n, c) for n in (4, 8, 13) for c in ("f32", "f64")])
def test_step_k_and_step_ex_at_every_threshold(amd, oracle_mod, n, commands):
    """step_k(K = 2, tape_out=True) and two step_ex() calls with defaults, each against the oracle (every step's outputs, the
    state after the second step: a hard collision counted once) and bit for bit against two step() calls, in every output and in
    state (step_kernel, step_k_kernel and step_ex_kernel each inline step_agent and the scans)."""
    import torch
    worst = [0.0, 0.0]
    for world in _worlds(n):
        b = tl.make_threshold_batch(n, world, commands)
        envs = [_device(amd, b) for _ in range(3)]
        orc = tl.oracle_for(oracle_mod, b)
        act = torch.from_numpy(np.ascontiguousarray(_commands(b))).to(envs[0].device)
        tape = torch.stack([act, act]).contiguous()
        ref = []
        for k in range(2):
            o, r, d, _ = envs[0].step(tape[k])
            ref.append((_np(o).copy(), _np(r).copy(), _np(d).copy()))
        ko, kr, kd, _ = envs[1].step_k(tape, tape_out=True)
        ko, kr, kd = _np(ko), _np(kr), _np(kd)
        for k in range(2):
            eo, er, ed, _ = envs[2].step_ex(tape[k])
            out_o = orc.step(b["act"])
            for name, got in (("step_k", (ko[k], kr[k], kd[k])), ("step_ex", (_np(eo), _np(er), _np(ed)))):
                ctx = f"{name} n={n} {world} {commands} step {k + 1}"
                e = _check_outputs(b, got, out_o, ctx)
                worst = [max(worst[0], e[0]), max(worst[1], e[1])]
                _same(b, got[0].view(np.uint32), ref[k][0].view(np.uint32), ctx + " obs against step()")
                _same(b, got[1].view(np.uint32), ref[k][1].view(np.uint32), ctx + " rew against step()")
                _same(b, got[2].astype(bool), ref[k][2].astype(bool), ctx + " done against step()")
        want = orc.get_state()
        s = [{k: _np(v) for k, v in e.get_state().items()} for e in envs]
        for j, name in ((1, "step_k"), (2, "step_ex")):
            ctx = f"{name} n={n} {world} {commands} state after two steps"
            for key in ("flags", "loc", "prev_d"):
                _same(b, s[j][key], want[key], f"{ctx} {key}")
            _same(b, s[j]["vel"].view(np.uint64), want["vel"].view(np.uint64), ctx + " vel (float64 bits)")
            _same(b, (s[j]["counters"][:, :3] != want["counters"][:, :3].astype(np.int32)).any(-1), False, ctx + " counters")
            for key in s[0]:
                bad = s[j][key] != s[0][key]
                assert not bad.any(), f"{ctx} {key} against step(): {_where(b, bad if key != 'counters' else bad.any(-1))}"
        for e in envs:
            e.close()
    print(f"step_k / step_ex n={n} {commands}: worst obs error {worst[0]:.3g}, worst reward error {worst[1]:.3g}; "
          f"bit-identical to step()")


@pytest.mark.parametrize("n,commands", [(1, "f64"), (1, "f32"), (4, "f64"), (8, "f32")])
def test_step_ex_auto_reset_follows_the_threshold(amd, oracle_mod, n, commands):
    """auto_reset="agent0_done": the G / S / O members in agent 0 that finish or leave are exactly the envs the next call
    re-initialises.  With step_cap = 2 every other env ends in the second call.  All against the oracle's step_ex."""
    worst = [0.0, 0.0]
    for world in ("r03", "r07"):
        b = tl.make_threshold_batch(n, world, commands)
        E = b["loc"].shape[0]
        ends = np.zeros(E, bool)
        for g in b["egos"]:
            if g["agent"] == 0 and g["cls"] in ("G", "S", "O"):
                ends[g["env"]] = g["expect"]
        assert ends.any() and not ends.all()
        for cap in (0, 2):
            env, orc = _device(amd, b), tl.oracle_for(oracle_mod, b)
            for t in (1, 2, 3):
                og, rg, dg, info = env.step_ex(_commands(b), auto_reset="agent0_done", step_cap=cap)
                oo, ro, do, rm, en, tr = orc.step_ex(b["act"], reset_policy=1, step_cap=cap, track_returns=True, seed=11,
                                                     with_end=True)
                ctx = f"step_ex call {t} n={n} {world} {commands} cap={cap}"
                _same(b, _np(info["reset_mask"]).astype(np.uint8), rm, ctx + " reset_mask")
                _same(b, _np(info["ended"]).astype(np.uint8), en, ctx + " ended")
                _same(b, _np(info["truncated"]).astype(np.uint8), tr, ctx + " truncated")
                if t == 1:
                    _same(b, en.astype(bool), ends, ctx + " ended by the threshold")
                if t == 2:
                    _same(b, rm.astype(bool), ends, ctx + " re-initialised")
                    if cap:
                        _same(b, en.astype(bool), ~ends, ctx + " ended by the cap (or, coasting on, by the box)")
                e = _check(b, env, orc, (og, rg, dg), (oo, ro, do), ctx)
                worst = [max(worst[0], e[0]), max(worst[1], e[1])]
            env.close()
    print(f"step_ex auto-reset n={n} {commands}: worst obs error {worst[0]:.3g}, worst reward error {worst[1]:.3g}")


@pytest.mark.parametrize("n", [7, 24])
def test_launch_shape_independence(amd, monkeypatch, n):
    """UAVX_GW = 1, 2, 3, 4 wavefronts per workgroup: bit-identical outputs and state, while the threshold egos change wavefront
    and the wavefronts their number of tied lanes (test_threshold_layouts_host.py checks that on the model)."""
    for world in _worlds(n):
        b = tl.make_threshold_batch(n, world, "f64")
        assert len({tuple(tl.ego_lanes(b, W)) for W in (1, 2, 3, 4)}) >= 3
        ref = None
        for W in (1, 2, 3, 4):
            monkeypatch.setenv("UAVX_GW", str(W))
            env = _device(amd, b)
            got = {}
            for t in (1, 2):
                o, r, d, _ = env.step(b["act"])
                got.update({f"obs{t}": _np(o).copy(), f"rew{t}": _np(r).copy(), f"done{t}": _np(d).copy()})
            got.update({"state " + k: _np(v) for k, v in env.get_state().items()})
            env.close()
            ref = ref or got
            for k in ref:
                bad = got[k] != ref[k]
                assert not bad.any(), f"n={n} {world} UAVX_GW={W} {k}: {_where(b, bad if 'counters' not in k else bad.any(-1))}"
    print(f"launch shapes n={n}: bit-identical")


# ---------------------------------------------------------------------------------------------------------------------------
# scripted bodies and levels; float64 positions
@pytest.mark.parametrize("L,B,leveled", [(4, 4, True), (8, 16, True), (4, 4, False), (8, 16, False)])
def test_bodies_and_levels_at_every_threshold(amd, oracle_mod, L, B, leveled):
    """C / CS / H between a learner and a body held still (the `body` visits of the scans), G and O of the learners; with levels,
    envs of two levels with different collider_radius, d_sense and box alternate inside every wavefront, each env's members at
    its own level's limits, where the other level's limits answer the other way round.  step() twice, and two step_ex() calls
    bit-identical to them.  The oracle's extension part restates this build's own definition of bodies and levels (DESIGN
    section 3); the limits under test are the reference's."""
    import torch
    b = tl.make_ext_batch(L, B, leveled)
    E = b["loc"].shape[0]
    kw = tl.ext_kwargs(b)
    env = tl.ext_setup(amd.BatchedMultiUAVWorld2D(E, seed=13, **kw), b)
    twin = tl.ext_setup(amd.BatchedMultiUAVWorld2D(E, seed=13, **kw), b)
    orc = tl.ext_setup(oracle_mod.OracleMulti(num_envs=E, nthreads=8, **kw), b)
    if leveled:
        _same(b, _np(env.env_levels()), b["level"], "levels")
    worst = [0.0, 0.0]
    act = torch.zeros((E, L, 2), dtype=torch.float32, device=env.device)
    for t in (1, 2):
        og, rg, dg, _ = env.step(act)
        ctx = f"step {t} {L}+{B} leveled={leveled}"
        e = _check(b, env, orc, (og, rg, dg), orc.step(b["act"]), ctx)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        _same(b, (_np(env.get_bodies()) != orc.body).any((1, 2)), False, ctx + " bodies")
        eo, er, ed, _ = twin.step_ex(act)
        _same(b, _np(eo).view(np.uint32), _np(og).view(np.uint32), ctx + " step_ex obs")
        _same(b, _np(er).view(np.uint32), _np(rg).view(np.uint32), ctx + " step_ex rew")
        _same(b, _np(ed), _np(dg), ctx + " step_ex done")
    for k, v in env.get_state().items():
        bad = _np(v) != _np(twin.get_state()[k])
        assert not bad.any(), f"step_ex state {k}: {_where(b, bad if k != 'counters' else bad.any(-1))}"
    env.close()
    twin.close()
    print(f"bodies / levels {L}+{B} leveled={leveled}: worst obs error {worst[0]:.3g}, worst reward error {worst[1]:.3g}")


def test_float64_positions_at_every_threshold(amd, oracle_mod):
    """float64-position mode at n = 3: distance 2R, 1.0, 0.5, speed 0.2 and the box halves, each at the Python float and one
    float64 step either side.  Everything bit for bit (positions, distances and velocities as float64) except observations and
    the float32 reward."""
    b = tl.make_threshold_batch64()
    E, n = b["loc"].shape[:2]
    env = amd.BatchedMultiUAVWorld2D(E, num_agents=n, seed=12, max_speed=tl.VMAX, max_acceleration=tl.AMAX, **tl.WORLD64)
    env.reset()
    env.set_state(vel=b["vel"])
    env.set_state_f64(loc=b["loc"], tgt=b["tgt"], init_d=b["init_d"], prev_d=b["prev_d"])
    assert env.position_mode == "float64"
    orc = tl.oracle_for64(oracle_mod, b)
    worst = [0.0, 0.0]
    name = lambda bad: [(b["egos"][e]["cls"], b["egos"][e]["member"], b["egos"][e]["agent"]) for e in np.flatnonzero(bad)[:4]]
    for t in (1, 2):
        og, rg, dg, _ = env.step(b["act"])
        oo, ro, do = orc.step(b["act"])
        ctx = f"float64 positions step {t}"
        bad = (_np(dg).astype(np.uint8) != do).any(1)
        assert not bad.any(), f"{ctx} done: {name(bad)}"
        s64 = {k: _np(v) for k, v in env.get_state_f64().items()}
        st = {k: _np(v) for k, v in env.get_state().items()}
        for k, got, ref in (("loc", s64["loc"], orc.loc), ("prev_d", s64["prev_d"], orc.prev_d), ("vel", st["vel"], orc.vel)):
            bad = (got.view(np.uint64) != ref.view(np.uint64)).reshape(E, -1).any(1)
            assert not bad.any(), f"{ctx} {k}: {name(bad)}"
        bad = (st["flags"] != orc.flags).any(1) | (st["counters"][:, :3] != orc.counters[:, :3].astype(np.int32)).any(1)
        assert not bad.any(), f"{ctx} flags / counters: {name(bad)}"
        oerr = obs_err(_np(og), oo)
        rerr = np.abs(_np(rg).astype(np.float64) - ro)
        assert oerr <= TOL, f"{ctx} obs {oerr:.3g}"
        assert rerr.max() <= TOL, f"{ctx} reward: {name((rerr > TOL).any(1))}"
        worst = [max(worst[0], oerr), max(worst[1], float(rerr.max()))]
    env.close()
    print(f"float64 positions: worst obs error {worst[0]:.3g}, worst reward error {worst[1]:.3g}")


# ---------------------------------------------------------------------------------------------------------------------------
# single-UAV world
def _uw_check(b, env, orc, out_g, out_o, ctx):
    (og, rg, dg, ig), (oo, ro, do, io) = out_g, out_o
    tag = lambda bad: [(b["egos"][e]["cls"], b["egos"][e]["member"]) for e in np.flatnonzero(bad)[:4]]
    bad = _np(dg).astype(np.uint8) != do
    assert not bad.any(), f"{ctx} done: {tag(bad)}"
    st = {k: _np(v) for k, v in env.get_state().items()}
    for k, ref in (("loc", orc.loc.astype(F32)), ("prev_d", orc.prev_d.astype(F32)), ("flags", orc.vel_f32 * 4)):
        bad = st[k] != ref
        assert not bad.any(), f"{ctx} {k}: {tag(bad.reshape(len(do), -1).any(1))}"
    bad = (st["vel"].view(np.uint64) != orc.vel.view(np.uint64)).any(1)
    assert not bad.any(), f"{ctx} vel: {tag(bad)}"
    bad = _np(ig["distance"]) != io.astype(F32)
    assert not bad.any(), f"{ctx} distance: {tag(bad)}"
    oerr = obs_err(_np(og), oo, (1, 3))
    assert oerr <= TOL, f"{ctx} obs {oerr:.3g}"
    rerr = np.abs(_np(rg).astype(np.float64) - ro)
    tol_r = np.maximum(TOL, np.spacing(np.abs(ro).astype(F32)).astype(np.float64))   # +1000 is a float32 sum in the reference
    assert (rerr <= tol_r).all(), f"{ctx} reward: {tag(rerr > tol_r)}"
    return oerr, float(rerr.max())


def _uw_pair(amd, oracle_mod, b):
    E = b["loc"].shape[0]
    env = amd.BatchedUAVWorld2D(E, seed=5, **tl.UW_BOXES[b["box"]])
    env.reset()
    env.set_state(loc=b["loc"], vel=b["vel"], tgt=b["tgt"], init_d=b["init_d"], prev_d=b["prev_d"], flags=b["vel_f32"] * 4)
    return env, tl.uw_oracle_for(oracle_mod, b)


@pytest.mark.parametrize("box,commands,fresh", [(x, c, f) for x in tl.UW_BOXES for c in ("f32", "f64") for f in (True, False)])
def test_single_uav_world_at_every_threshold(amd, oracle_mod, box, commands, fresh):
    b = tl.make_uw_batch(box, commands, fresh)
    act = _commands(b)
    worst = [0.0, 0.0]
    env, orc = _uw_pair(amd, oracle_mod, b)
    for t in (1, 2):
        e = _uw_check(b, env, orc, env.step(act), orc.step(act), f"uw step {t} {box} {commands} fresh={fresh}")
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    env.close()
    ends = np.array([g["expect"] for g in b["egos"]])
    for cap in (0, 2):
        env, orc = _uw_pair(amd, oracle_mod, b)
        for t in (1, 2, 3):
            og, rg, dg, info = env.step_ex(act, auto_reset=True, step_cap=cap)
            oo, ro, do, io, rm = orc.step_ex(act, auto_reset=True, step_cap=cap, seed=5)
            ctx = f"uw step_ex call {t} {box} {commands} fresh={fresh} cap={cap}"
            assert np.array_equal(_np(info["reset_mask"]).astype(np.uint8), rm), ctx
            if t == 1:
                assert np.array_equal(do.astype(bool), ends), ctx
            if t == 2:
                assert np.array_equal(rm.astype(bool), ends), ctx                  # exactly the members past their threshold
            if t == 3 and cap:
                assert np.array_equal(rm.astype(bool), ~ends), ctx                 # the others were cut by the cap in call 2
            e = _uw_check(b, env, orc, (og, rg, dg, info), (oo, ro, do, io), ctx)
            worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        env.close()
    print(f"single-UAV {box} {commands} fresh={fresh}: worst obs error {worst[0]:.3g}, worst reward error {worst[1]:.3g}")

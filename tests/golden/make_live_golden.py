#!/usr/bin/env python3
"""Records the REFERENCE env's side of tests/test_reference_live.py into tests/golden/live_*.npz.

Run where the reference checkout is importable (see ref_loader.py):
    python tests/golden/make_live_golden.py              (everything)
    python tests/golden/make_live_golden.py thresholds   (live_thresholds.npz alone; likewise signed_zero)
Each scenario of the three live cross-checks (seeds, agent counts, the actions fed, evaluate flags) is driven through the
reference exactly as the tests drive the oracle, and what the tests compare is stored: the commands, the reference's
observations after every reset, and per step its dones, positions, velocities, previous distances, flags, counters,
rewards and observations.  Data only; the tests then need nothing outside the repository.
"""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

# the scenarios of tests/test_reference_live.py (that module imports these lists)
MUW_CASES = [(1, 101), (2, 102), (3, 103), (4, 104), (4, 105), (7, 106), (12, 107), (20, 108)]
MUW_EPISODES, MUW_T = 3, 150
UW_SEEDS = [201, 202]
UW_EPISODES, UW_T = 3, 200
F64_CASES = [(4, True), (6, True), (5, False), (3, False)]
F64_T = 900


def muw_kwargs(n, seed):
    return dict(num_agents=n) if seed % 2 else dict(num_agents=n, x_size=30.0, y_size=36.0, d_sense=9, collider_radius=0.8)


def snap(env):
    ags = env.agent_list
    return dict(loc=np.array([a.location for a in ags], np.float64), vel=np.array([a.velocity for a in ags], np.float64),
                prev_d=np.array([a.prev_distance for a in ags], np.float64),
                flags=np.array([(1 if a.done else 0) | (2 if a.collided else 0) for a in ags], np.uint8),
                counters=np.array([env.steps, env.target_reach_count, env.collision_count], np.uint32))


def record(rows, **fields):
    for k, v in fields.items():
        rows.setdefault(k, []).append(np.asarray(v))


def save(name, data, meta):
    meta = dict(meta, numpy=np.__version__, generator="tests/golden/make_live_golden.py")
    data = {k: np.stack(v) if isinstance(v, list) else v for k, v in data.items()}
    data["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **data)


def make_muw(MUW):
    for n, seed in MUW_CASES:
        np.random.seed(seed)
        env = MUW(**muw_kwargs(n, seed))
        rng = np.random.default_rng(seed)
        rows = {}
        for _ in range(MUW_EPISODES):
            record(rows, reset_obs=np.array(env.reset(), np.float64))
            for t in range(MUW_T):
                if t % 3 == 0:
                    acts = [rng.uniform(-10, 10, 2).astype(np.float32) for _ in range(n)]
                else:  # goal seeking, float64 like the trainers' converted actions
                    acts = []
                    for a in env.agent_list:
                        d = np.asarray(a.target_location, np.float64) - np.asarray(a.location, np.float64)
                        dist = float(np.linalg.norm(d))
                        acts.append(d / max(dist, 1e-9) * (min(8.0, math.sqrt(4 * dist)) if dist > 0.3 else 0.0))
                act = np.array(acts, np.float64)
                obs, rew, done, _ = env.step(acts, evaluate=bool(t % 7 == 0))
                record(rows, actions=act, done=np.array(done, np.uint8), rew=np.array([float(r) for r in rew]),
                       obs=np.array(obs, np.float64), **snap(env))
        save(f"live_muw_n{n}_s{seed}", rows, dict(kind="live_muw", n=n, seed=seed, episodes=MUW_EPISODES, T=MUW_T,
                                                   kwargs=muw_kwargs(n, seed)))


def make_uw(UW):
    for seed in UW_SEEDS:
        np.random.seed(seed)
        env = UW()
        rng = np.random.default_rng(seed)
        rows = {}
        for _ in range(UW_EPISODES):
            record(rows, reset_obs=np.asarray(env.reset(), np.float64))
            for t in range(UW_T):
                a = rng.uniform(-12, 12, 2).astype(np.float32) if (t + seed) % 2 else rng.uniform(-12, 12, 2)
                obs, rew, done, info = env.step(a)
                record(rows, done=np.uint8(bool(done)), rew=np.float64(rew), distance=np.float64(info["distance"]),
                       obs=np.asarray(obs, np.float64), loc=np.asarray(env._agent_location, np.float64),
                       vel=np.asarray(env._agent_speed, np.float64))
        save(f"live_uw_s{seed}", rows, dict(kind="live_uw", seed=seed, episodes=UW_EPISODES, T=UW_T))


def f64_actions(env, t):
    acts = []
    for a in env.agent_list:
        d = np.asarray(a.target_location, np.float64) - np.asarray(a.location, np.float64)
        acts.append(d * 1.5 if (t % 5 or t > 150) else d * 1.5 + np.array([0.3, -0.2]))
    return acts


def make_f64(MUW):
    for n, circular in F64_CASES:
        np.random.seed(300 + n)
        env = MUW(num_agents=n)
        rows = {"reset_obs": np.array(env.reset(circular=circular), np.float64)}
        if not circular:   # the plotting script's float64 pokes (test_sac_multi_plot_trajectory.py:43-49)
            for i in range(n):
                theta = 2 * i * math.pi / n
                env.agent_list[i].location = 20 * np.ones(2) * np.array([math.cos(theta), math.sin(theta)])
                env.agent_list[i].target_location = 23 * np.ones(2) * np.array([math.cos(theta + math.pi - 0.5 * math.pi / n),
                                                                              math.sin(theta + math.pi - 0.5 * math.pi / n)])
            rows["poked_loc"] = np.array([a.location for a in env.agent_list], np.float64)
            rows["poked_tgt"] = np.array([a.target_location for a in env.agent_list], np.float64)
        for t in range(F64_T):
            acts = f64_actions(env, t)
            obs, rew, done, _ = env.step(acts, evaluate=bool(t % 11 == 0))
            record(rows, actions=np.array(acts, np.float64), done=np.array(done, np.uint8),
                   rew=np.array([float(r) for r in rew]), obs=np.array(obs, np.float64), **snap(env))
        save(f"live_f64_n{n}_{'circular' if circular else 'poked'}", rows,
             dict(kind="live_f64", n=n, circular=circular, T=F64_T))


# signed zeros: velocities / target offsets / neighbour offsets of (+-0, +-0) poked into a 4-agent world
SZ_CASES = [(-0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (0.0, 0.0)]


def signed_zero_state(k):
    """Scenario k of make_signed_zero: float32 locations and targets, float64 velocities, done flags (agent 3 is done when
    k is odd and agent 2 then sits at (-0, -0), on top of agent 0)."""
    z, m = 0.0, -0.0
    loc = np.array([[z, z], [6.0, 1.0], [-5.0, 7.0], [2.0, z]], np.float32)
    vx, vy = SZ_CASES[k % 4]
    tx, ty = SZ_CASES[(k // 4) % 4]
    vel = np.array([[vx, vy], [1.0, 2.0], [vx, vy], list(SZ_CASES[(k + 1) % 4])], np.float64)
    tgt = np.array([[tx, ty], [20.0, 20.0], [-20.0, 9.0], [30.0, -30.0]], np.float32)
    done = np.array([0, 0, 0, k % 2], np.uint8)
    if k % 2:
        loc[2] = [m, m]
    return loc, vel, tgt, done


def make_signed_zero(MUW):
    rows = {}
    for k in range(16):
        np.random.seed(400 + k)
        env = MUW(num_agents=4)
        env.reset()
        loc, vel, tgt, done = signed_zero_state(k)
        for i, a in enumerate(env.agent_list):
            a.location, a.velocity, a.target_location, a.done = loc[i].copy(), vel[i].copy(), tgt[i].copy(), bool(done[i])
        record(rows, obs=np.array([env._get_obs(a) for a in env.agent_list], np.float64))
    save("live_signed_zero", rows, dict(kind="live_signed_zero", cases=16))


# the reference's verdict at the step thresholds: one single-env world per class member of tests/threshold_layouts.py
THR_AGENTS = (2, 3)
THR_COMMANDS = ("f64", "f32")


def thr_groups():
    """(key, kind, args) of every group of live_thresholds.npz (tests/test_threshold_layouts_host.py imports this)."""
    sys.path.insert(0, os.path.dirname(HERE))
    import threshold_layouts as tl
    out = [(f"muw_n{n}_{w}_{c}", "muw", (n, w, c)) for n in THR_AGENTS for w in tl.WORLDS for c in THR_COMMANDS]
    out += [(f"uw_{b}_{c}_{'fresh' if f else 'later'}", "uw", (b, c, f)) for b in tl.UW_BOXES for c in THR_COMMANDS
            for f in (False, True)]
    return tl, out


def make_thresholds(MUW, UW):
    """Pokes the crafted state of every class member (section 0 of the batch) into a fresh reference world and records two
    steps with evaluate=False and, from the same state again, one with evaluate=True."""
    tl, groups = thr_groups()
    data = {}
    for key, kind, args in groups:
        rows = {}
        if kind == "muw":
            n, world, cmd = args
            b = tl.make_threshold_batch(n, world, cmd)
            envs = np.flatnonzero((b["section"] == 0) & ~b["filler"])
            for e in envs:
                for ev in (False, True):
                    np.random.seed(500 + int(e))
                    env = MUW(num_agents=n, **tl.WORLDS[world])
                    env.reset()
                    for i, a in enumerate(env.agent_list):
                        a.location, a.target_location = b["loc"][e, i].copy(), b["tgt"][e, i].copy()
                        a.velocity, a.velocity_prev = b["vel"][e, i].copy(), b["vel"][e, i].copy()
                        a.init_distance, a.prev_distance = b["init_d"][e, i], b["prev_d"][e, i]
                    act = b["act32"][e] if cmd == "f32" else b["act"][e]
                    for t in range(1 if ev else 2):
                        _, rew, done, _ = env.step([act[i].copy() for i in range(n)], evaluate=ev)
                        tag = "eval" if ev else f"step{t + 1}"
                        record(rows, **{f"{tag}_{k}": v for k, v in dict(snap(env), done=np.array(done, np.uint8),
                                                                          rew=np.array([float(r) for r in rew])).items()})
            rows["env"] = envs
            for k in ("loc", "vel", "tgt", "init_d", "prev_d", "act"):
                rows["in_" + k] = b[k][envs]
        else:
            box, cmd, fresh = args
            b = tl.make_uw_batch(box, cmd, fresh)
            for e in range(b["loc"].shape[0]):
                np.random.seed(600 + e)
                env = UW(**tl.UW_BOXES[box])
                env.reset()
                env._agent_location, env._target_location = b["loc"][e].copy(), b["tgt"][e].copy()
                vel = b["vel"][e].astype(np.float32) if fresh else b["vel"][e].copy()
                env._agent_speed = env._agent_speed_prev = vel
                env._init_target_distance, env._prev_distance = b["init_d"][e], b["prev_d"][e]
                act = b["act32"][e] if cmd == "f32" else b["act"][e]
                for t in range(2):
                    obs, rew, done, info = env.step(act.copy())
                    record(rows, **{f"step{t + 1}_{k}": v for k, v in dict(
                        done=np.uint8(bool(done)), rew=np.float64(rew), distance=np.float64(info["distance"]),
                        obs=np.asarray(obs, np.float64), loc=np.asarray(env._agent_location, np.float64),
                        vel=np.asarray(env._agent_speed, np.float64)).items()})
            for k in ("loc", "vel", "tgt", "init_d", "prev_d", "act"):
                rows["in_" + k] = b[k]
        for k, v in rows.items():
            data[f"{key}__{k}"] = np.stack(v) if isinstance(v, list) else v
    save("live_thresholds", data, dict(kind="live_thresholds", groups=[g[0] for g in groups]))


if __name__ == "__main__":
    MUW, UW, _ = ref_loader.load()
    if sys.argv[1:] == ["signed_zero"]:
        make_signed_zero(MUW)
        sys.exit(0)
    if sys.argv[1:] == ["thresholds"]:
        make_thresholds(MUW, UW)
        sys.exit(0)
    make_muw(MUW)
    make_uw(UW)
    make_f64(MUW)
    make_signed_zero(MUW)
    make_thresholds(MUW, UW)

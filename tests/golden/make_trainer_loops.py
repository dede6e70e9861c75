#!/usr/bin/env python3
"""Records the reference trainers' rollout loop into tests/golden/trainer_loop_{muw,uw}.npz.

Run where the reference checkout is importable (see ref_loader.py):
    python tests/golden/make_trainer_loops.py
The loop is the training branch of test_sac_multi.py:62-119 (MultiUAVWorld2D, 4 agents) and test_sac.py:68-110
(UAVWorld2D): np.random.seed(s), env.reset(return_info=True); warm-up actions np.random.uniform(-1, 1, (2,)) per agent from
the global stream the resets draw from (float64); after WARM_UP total steps the actions of a seeded CPU
policy.GaussianPolicy (float32, tanh(mean)); the literal polar conversion of the trainers; env.step; break on dones[0]
(done) or on the step cap; the counters are read, then env.reset().  Stored, flat over all steps of all episodes:
  ep_start [episodes + 1]        first step of each episode (and the total)
  init_*  [episodes, ...]        the full state after each reset (what set_state / the counters need), reset_obs
  act [steps, (N,) 2] float64    the raw action, exactly widened; act_f64 [steps] marks the float64 (warm-up) steps
  cmd [steps, (N,) 2] float64    the converted command (exactly widened when it is float32); cmd_f64 [steps]
  obs / rew / done               s' , r and done of every step (s of step t is obs[t-1], or reset_obs at an episode start)
  loc / vel / prev_d / flags     the state after every step; counters (MUW: steps, reach, collisions) before each reset
Data only: no reference source in any form.
"""
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_loader  # noqa: E402
from gym_uav_collision_avoidance_amd.policy import GaussianPolicy  # noqa: E402

EPISODES = 24
STEP_CAP = 90
MUW_SEED, UW_SEED, POLICY_SEED = 4242, 4343, 7
MUW_WARM_UP, UW_WARM_UP = 700, 900      # total steps: both land in the middle of an episode
CITED = {"trainer_loop_muw": "test_sac_multi.py:62-119 (conversion :77-80)", "trainer_loop_uw": "test_sac.py:68-110 (conversion :77-78)"}


def policy(num_inputs):
    torch.manual_seed(POLICY_SEED)
    pol = GaussianPolicy(num_inputs, 2, hidden=64).eval()
    return lambda s: pol.act(torch.as_tensor(np.asarray(s, np.float32)), evaluate=True).numpy()   # float32, tanh(mean)


def convert(action, scale):
    """The trainers' literal expression (scale: np.linalg.norm(env.action_space.high) or env.action_space.high[0])."""
    v = (action[0] / 2 + 0.5) * scale
    theta = action[1] * math.pi
    return np.array([v * math.cos(theta), v * math.sin(theta)])


def record(rows, **fields):
    for k, v in fields.items():
        rows.setdefault(k, []).append(np.asarray(v))


def muw_state(env):
    ags = env.agent_list
    return dict(loc=np.array([a.location for a in ags], np.float64), vel=np.array([a.velocity_prev for a in ags], np.float64),
                tgt=np.array([a.target_location for a in ags], np.float64),
                init_d=np.array([a.init_distance for a in ags], np.float64),
                prev_d=np.array([a.prev_distance for a in ags], np.float64),
                flags=np.array([(1 if a.done else 0) | (2 if a.collided else 0) for a in ags], np.uint8))


def make_muw(MUW, n=4):
    np.random.seed(MUW_SEED)
    env = MUW(num_agents=n)
    scale = np.linalg.norm(env.action_space.high)
    act_fn = policy(10)
    rows, ep_start, total = {}, [], 0
    states, _ = env.reset(return_info=True)
    for _ in range(EPISODES):
        ep_start.append(len(rows.get("rew", [])))
        st = muw_state(env)
        record(rows, **{"init_" + k: v for k, v in st.items()}, reset_obs=np.array(states, np.float64),
               init_counters=np.array([env.steps, env.target_reach_count, env.collision_count], np.int64))
        for _step in range(STEP_CAP):
            acts, cmds = [], []
            for i in range(n):
                action = np.random.uniform(low=-1, high=1, size=(2,)) if total < MUW_WARM_UP else act_fn(states[i])
                acts.append(action)
                cmds.append(convert(action, scale))
            next_states, rewards, dones, _ = env.step(cmds)
            st = muw_state(env)
            record(rows, act=np.array(acts, np.float64), act_f64=acts[0].dtype == np.float64,
                   cmd=np.array(cmds, np.float64), cmd_f64=cmds[0].dtype == np.float64,
                   obs=np.array(next_states, np.float64), rew=np.array([float(r) for r in rewards]),
                   done=np.array(dones, np.uint8), loc=st["loc"], vel=st["vel"], prev_d=st["prev_d"], flags=st["flags"])
            states = next_states
            total += 1
            if dones[0]:
                break
        record(rows, counters=np.array([env.steps, env.target_reach_count, env.collision_count], np.int64))
        states, _ = env.reset(return_info=True)
    ep_start.append(len(rows["rew"]))
    return rows, ep_start, dict(kind="trainer_loop_muw", num_agents=n, seed=MUW_SEED, warm_up=MUW_WARM_UP, scale=float(scale))


def make_uw(UW):
    np.random.seed(UW_SEED)
    env = UW()
    scale = env.action_space.high[0]
    act_fn = policy(4)
    rows, ep_start, total = {}, [], 0
    state, _ = env.reset(return_info=True)
    for _ in range(EPISODES):
        ep_start.append(len(rows.get("rew", [])))
        record(rows, init_loc=np.asarray(env._agent_location, np.float64), init_vel=np.asarray(env._agent_speed_prev, np.float64),
               init_vel_f32=np.asarray(env._agent_speed_prev).dtype == np.float32,
               init_tgt=np.asarray(env._target_location, np.float64), init_init_d=np.float64(env._init_target_distance),
               init_prev_d=np.float64(env._prev_distance), init_steps=np.int64(env.steps), reset_obs=np.asarray(state, np.float64))
        for _step in range(STEP_CAP):
            action = np.random.uniform(low=-1, high=1, size=(2,)) if total < UW_WARM_UP else act_fn(state)
            cmd = convert(action, scale)
            next_state, reward, done, info = env.step(cmd)
            record(rows, act=np.asarray(action, np.float64), act_f64=action.dtype == np.float64, cmd=np.asarray(cmd, np.float64),
                   cmd_f64=cmd.dtype == np.float64, obs=np.asarray(next_state, np.float64), rew=np.float64(reward),
                   done=np.uint8(bool(done)), distance=np.float64(info["distance"]),
                   loc=np.asarray(env._agent_location, np.float64), vel=np.asarray(env._agent_speed, np.float64))
            state = next_state
            total += 1
            if done:
                break
        record(rows, counters=np.array([env.steps], np.int64))
        state, _ = env.reset(return_info=True)
    ep_start.append(len(rows["rew"]))
    return rows, ep_start, dict(kind="trainer_loop_uw", seed=UW_SEED, warm_up=UW_WARM_UP, scale=float(scale))


def save(name, rows, ep_start, meta):
    meta = dict(meta, numpy=np.__version__, episodes=EPISODES, step_cap=STEP_CAP, policy_seed=POLICY_SEED,
                policy="policy.GaussianPolicy(hidden=64), torch.manual_seed(policy_seed), act(evaluate=True)",
                cited=CITED[meta["kind"]], generator="tests/golden/make_trainer_loops.py")
    data = {k: np.stack(v) for k, v in rows.items()}
    data["ep_start"] = np.array(ep_start, np.int64)
    data["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes,", int(ep_start[-1]), "steps,", int(data["act_f64"].sum()), "float64-action steps")


if __name__ == "__main__":
    MUW, UW, _ = ref_loader.load()
    save("trainer_loop_muw", *make_muw(MUW))
    save("trainer_loop_uw", *make_uw(UW))

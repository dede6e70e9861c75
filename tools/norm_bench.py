#!/usr/bin/env python3
"""Times the running-statistics calls of RolloutNormalizer -- fold_obs, fold_returns, obs_ring and rewards --
against the same semantics composed from torch ops (masked float64 reductions for the statistics, a forward Python loop over
the steps for the returns), on the three rings of tools/gae_bench.py written by real env steps, in three alternating rounds
(min / median / max per case); every torch composition is timed as two cases, whose spread is the noise margin.  Then one
train_ppo.py iteration at 4 096 x 4 x 32 with the two switches off (twice) and on.

Writes profiles/norm_bench.json (one object) and prints it.

    python tools/norm_bench.py [--out profiles/norm_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from critic_bench import time_us                                                    # noqa: E402
from gae_bench import RINGS, rounds                                                 # noqa: E402
from prio_bench import ring                                                         # noqa: E402
from gym_uav_collision_avoidance_amd import UAVVectorEnv, _norm_lib                 # noqa: E402
from gym_uav_collision_avoidance_amd.normalize import RolloutNormalizer             # noqa: E402
from gym_uav_collision_avoidance_amd.ppo import PPO                                 # noqa: E402
from gym_uav_collision_avoidance_amd.replay import DeviceReplay                     # noqa: E402

GAMMA, EPS, CLIP = 0.99, 1e-8, 10.0
CALLS = ("fold_obs", "fold_returns", "obs_ring", "rewards")


class TorchNormalizer:
    """include/uavx_norm.h in torch ops (the order of the sums is torch's)."""

    def __init__(self, mem):
        self.mem = mem
        dev, (L, E, N, F) = mem.rew.device, mem.obs.shape
        f64 = dict(dtype=torch.float64, device=dev)
        self.n_obs, self.mean, self.M2 = torch.zeros((), **f64), torch.zeros(F, **f64), torch.zeros(F, **f64)
        self.n_ret, self.mean_ret, self.M2_ret = torch.zeros((), **f64), torch.zeros((), **f64), torch.zeros((), **f64)
        self.carry = torch.zeros((E, N), **f64)
        self.learner = (torch.arange(N, device=dev) < mem.num_learners)[None, None, :]
        self.zero = torch.zeros((), **f64)

    def samples(self, first, count):
        """(slots [steps], mask [steps, E, N]) of the fold."""
        mem = self.mem
        slots = torch.arange(first, count, device=mem.rew.device) % mem.L
        prev = (slots - 1) % mem.L
        sk, _, _ = mem._flags(slots, slice(None))
        skp, _, enp = mem._flags(prev, slice(None))
        parked = ((mem.done[prev] & 1) != 0) & ~(skp | enp).unsqueeze(-1)
        if first == 0:
            parked[0] = False
        return slots, ~sk.unsqueeze(-1) & ~parked & self.learner

    @staticmethod
    def merge(na, mean_a, M2_a, nb, mean_b, M2_b):
        n = na + nb
        w = nb / n.clamp(min=1)
        delta = mean_b - mean_a
        return n, mean_a + delta * w, M2_a + M2_b + delta * delta * (na * w)

    def batch(self, x, mask):
        """x [..., (F)] float64 with mask over its leading axes -> (n, mean, M2) over the masked entries."""
        dims = tuple(range(mask.dim()))
        m = mask if x.dim() == mask.dim() else mask.unsqueeze(-1)
        n = mask.sum().double()
        mean = torch.where(m, x, self.zero).sum(dims) / n.clamp(min=1)
        return n, mean, torch.where(m, (x - mean) ** 2, self.zero).sum(dims)

    def fold_obs(self, first, count):
        slots, mask = self.samples(first, count)
        nb, mean_b, M2_b = self.batch(self.mem.obs[slots].double(), mask)
        self.n_obs, self.mean, self.M2 = self.merge(self.n_obs, self.mean, self.M2, nb, mean_b, M2_b)

    def fold_returns(self, first, count):
        mem = self.mem
        slots, mask = self.samples(first, count)
        C, rows = self.carry, []
        for j, k in enumerate(range(first, count)):
            s = k % mem.L
            _, _, en = mem._flags(s, slice(None))
            R = mem.rew[s].double() + GAMMA * C
            rows.append(R)
            stop = ((mem.done[s] & 1) != 0) | en[:, None]
            C = torch.where(mask[j] & ~stop, R, self.zero)
        self.carry = C
        nb, mean_b, M2_b = self.batch(torch.stack(rows), mask)
        self.n_ret, self.mean_ret, self.M2_ret = self.merge(self.n_ret, self.mean_ret, self.M2_ret, nb, mean_b, M2_b)

    def obs_ring(self):
        var = torch.where(self.n_obs > 0, self.M2 / self.n_obs.clamp(min=1), torch.ones_like(self.M2))
        return ((self.mem.obs.double() - self.mean) / (var + EPS).sqrt()).float().clamp(-CLIP, CLIP)

    def rewards(self):
        var = torch.where(self.n_ret > 0, self.M2_ret / self.n_ret.clamp(min=1), torch.ones_like(self.M2_ret))
        return (self.mem.rew.double() / (var + EPS).sqrt()).float().clamp(-CLIP, CLIP)


def measure(envs, horizon, dev):
    env, mem = ring(envs, horizon, 50, dev)
    first, count = mem.count - horizon, mem.count
    hip, ref = RolloutNormalizer(mem, gamma=GAMMA, eps=EPS, clip_obs=CLIP, clip_reward=CLIP), TorchNormalizer(mem)

    def hip_fold(name):
        def call():
            hip.folded_obs = hip.folded_ret = first
            getattr(hip, name)()
        return call

    hip_fold("fold_obs")(), hip_fold("fold_returns")(), ref.fold_obs(first, count), ref.fold_returns(first, count)
    torch.cuda.synchronize()
    st = hip.stats
    samples = int(st.n_obs)
    rel = lambda a, b: float(((a - b).abs() / b.abs().clamp(min=1e-300)).max())
    agrees = dict(n_obs=int(st.n_obs) == int(ref.n_obs), n_ret=int(st.n_ret) == int(ref.n_ret),
                  mean_max_rel_diff=rel(st.mean, ref.mean), var_max_rel_diff=rel(st.var, ref.M2 / ref.n_obs),
                  var_ret_rel_diff=rel(st.var_ret, ref.M2_ret / ref.n_ret),
                  carry_max_abs_diff=float((hip.carry - ref.carry).abs().max()),
                  obs_ring_max_abs_diff=float((hip.obs_ring() - ref.obs_ring()).abs().max()),
                  rewards_max_abs_diff=float((hip.rewards() - ref.rewards()).abs().max()))
    fns = {"hip_fold_obs": hip_fold("fold_obs"), "hip_fold_returns": hip_fold("fold_returns"), "hip_obs_ring": hip.obs_ring,
           "hip_rewards": hip.rewards}
    for tag in ("a", "b"):
        fns.update({f"torch_fold_obs_{tag}": lambda: ref.fold_obs(first, count),
                    f"torch_fold_returns_{tag}": lambda: ref.fold_returns(first, count),
                    f"torch_obs_ring_{tag}": ref.obs_ring, f"torch_rewards_{tag}": ref.rewards})
    big = envs * horizon >= 1 << 20
    iters = {k: (200 if k.startswith("hip") else 3 if "fold_returns" in k else 10 if big else 30) for k in fns}
    res = rounds(fns, iters)
    for call in CALLS:
        a, b = res[f"torch_{call}_a"][1], res[f"torch_{call}_b"][1]
        res[f"{call}_noise_us"] = round(abs(a - b), 2)
        res[f"{call}_speedup"] = round(min(a, b) / res[f"hip_{call}"][1], 2)
        res[f"{call}_beats_torch_by_more_than_noise"] = bool(res[f"hip_{call}"][1] + abs(a - b) < min(a, b))
    res.update(envs=envs, agents=4, horizon=horizon, features=int(mem.obs.shape[-1]),
               sample_share=round(samples / (horizon * envs * 4), 4),
               agrees=agrees)
    env.close()
    return res


def ppo_iteration(dev, normalised, envs=4096, agents=4, rollout=32, iterations=5):
    """Median over `iterations` iterations of examples/train_ppo.py's loop, in µs: acting, stepping, the update."""
    torch.manual_seed(0)
    venv = UAVVectorEnv(envs, num_agents=agents, device=dev, seed=0)
    mem = DeviceReplay(venv.env, horizon=rollout)
    mem.begin(venv.reset())
    ppo = PPO(mem, generator=torch.Generator(device=dev).manual_seed(0), normalize_obs=normalised, normalize_reward=normalised)
    phases = {k: [] for k in ("acting", "stepping", "update")}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    for it in range(iterations + 1):
        marks = {k: [] for k in phases}
        for _ in range(rollout):
            marks["acting"].append(timed(ppo.act))
            marks["stepping"].append(timed(lambda: mem.step(polar=True, auto_reset="agent0_done", step_cap=1500)))
        marks["update"].append(timed(ppo.update))
        torch.cuda.synchronize()
        if it:                                        # the first iteration warms everything up
            for k, v in marks.items():
                phases[k].append(sum(a.elapsed_time(b) for a, b in v) * 1e3)
    med = {k: round(sorted(v)[len(v) // 2], 1) for k, v in phases.items()}
    med["iteration"] = round(sum(med.values()), 1)
    med.update(envs=envs, agents=agents, rollout=rollout, normalize_obs=normalised, normalize_reward=normalised)
    venv.close()
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(unit="us per call: [min, median, max] of 3 alternating rounds; eager calls, host launch cost included",
               gamma=GAMMA, eps=EPS, clip=CLIP, norm_sha=_norm_lib.source_hash(), device=torch.cuda.get_device_name(0),
               rings=[measure(envs, horizon, dev) for envs, horizon in RINGS],
               ppo_iteration_us=dict(off_a=ppo_iteration(dev, False), on=ppo_iteration(dev, True), off_b=ppo_iteration(dev, False)))
    text = json.dumps(res, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

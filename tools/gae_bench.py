#!/usr/bin/env python3
"""Times the GAE(λ) advantage pass over the device ring against the same semantics composed from torch ops
(a reverse Python loop over the window in float64), normalised and raw, on rings written by real env steps, in three
alternating rounds (min / median / max per case); the torch loop is timed as two cases, whose spread is the noise margin.
Then one train_ppo.py iteration at 4 096 x 4 x 32 split into acting, stepping, advantages and the torch update.

Writes profiles/gae_bench.json (one object) and prints it.

    python tools/gae_bench.py [--out profiles/gae_bench.json]
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
from prio_bench import ring                                                         # noqa: E402
from gym_uav_collision_avoidance_amd import UAVVectorEnv, _gae_lib                  # noqa: E402
from gym_uav_collision_avoidance_amd.ppo import PPO                                 # noqa: E402
from gym_uav_collision_avoidance_amd.replay import DeviceReplay                     # noqa: E402
from gym_uav_collision_avoidance_amd.rollout import RolloutAdvantages               # noqa: E402

GAMMA, LAM = 0.99, 0.95
RINGS = ((1024, 32), (1024, 256), (65536, 32))       # envs (x 4 agents), horizon


class TorchGAE:
    """include/uavx_gae.h in torch ops: one group of launches per step of the window."""

    def __init__(self, mem, normalize):
        self.mem, self.normalize = mem, normalize
        shape, dev = mem.rew.shape, mem.rew.device
        self.adv, self.ret = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
        self.valid = torch.zeros(shape, dtype=torch.uint8, device=dev)
        self.norm = torch.zeros(shape, device=dev)
        self.learner = (torch.arange(shape[2], device=dev) < mem.num_learners)[None, :]
        self.zero = torch.zeros((), dtype=torch.float64, device=dev)
        self.zero32 = torch.zeros((), device=dev)

    def __call__(self, values, steps):
        mem, L, count = self.mem, self.mem.L, self.mem.count
        carry = torch.zeros(mem.rew.shape[1:], dtype=torch.float64, device=values.device)
        cut = None
        for k in range(count - 1, count - steps - 1, -1):
            s, s1 = k % L, (k + 1) % L
            sk, _, en = mem._flags(s, slice(None))
            d = (mem.done[s] & 1) != 0
            V = values[s].double()
            b = torch.where(d, self.zero, GAMMA * values[s1].double())
            delta = (mem.rew[s].double() + b) - V
            stop = d | en[:, None]
            stop = torch.ones_like(stop) if cut is None else stop | cut[:, None]
            A = torch.where(stop, delta, delta + (GAMMA * LAM) * carry)
            live = ~sk[:, None] & self.learner
            self.adv[s] = torch.where(live, A.float(), self.zero32)
            self.ret[s] = torch.where(live, (A + V).float(), self.zero32)
            self.valid[s] = live
            carry = torch.where(sk[:, None], self.zero, A)
            cut = sk
        if self.normalize:
            slots = torch.arange(count - steps, count, device=values.device) % L
            a, v = self.adv[slots].double(), self.valid[slots] != 0
            n = v.sum()
            mean = torch.where(v, a, self.zero).sum() / n.clamp(min=1)
            var = torch.where(v, (a - mean) ** 2, self.zero).sum() / (n - 1).clamp(min=1)
            std = torch.where(n >= 2, var.sqrt(), self.zero)
            self.norm[slots] = torch.where(v, ((a - mean) / (std + 1e-8)).float(), self.zero32)
        return self.adv, self.ret, self.valid, self.norm


def rounds(fns, iters):
    """{name: [min, median, max]} of three alternating rounds; iters: {name: replays per timing}."""
    times = {name: [] for name in fns}
    for _ in range(3):
        for name, fn in fns.items():
            times[name].append(time_us(fn, iters[name]))
    return {k: [round(x, 2) for x in sorted(v)] for k, v in times.items()}


def measure(envs, horizon, dev):
    env, mem = ring(envs, horizon, 50, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    values = torch.randn(mem.rew.shape, generator=g, device=dev)
    steps = horizon
    hip = {True: RolloutAdvantages(mem, GAMMA, LAM, normalize=True), False: RolloutAdvantages(mem, GAMMA, LAM, normalize=False)}
    ref = {True: TorchGAE(mem, True), False: TorchGAE(mem, False)}
    out, want = hip[True].compute(values, steps), ref[True](values, steps)
    slots = hip[True].window(steps)
    torch.cuda.synchronize()
    agrees = dict(adv=bool(torch.equal(out.adv[slots], want[0][slots])), ret=bool(torch.equal(out.ret[slots], want[1][slots])),
                  valid=bool(torch.equal(out.valid[slots], want[2][slots])),
                  adv_norm_max_abs_diff=float((out.adv_norm[slots] - want[3][slots]).abs().max()))
    fns = {"hip_norm": lambda: hip[True].compute(values, steps), "hip_raw": lambda: hip[False].compute(values, steps),
           "torch_norm_a": lambda: ref[True](values, steps), "torch_raw_a": lambda: ref[False](values, steps),
           "torch_norm_b": lambda: ref[True](values, steps), "torch_raw_b": lambda: ref[False](values, steps)}
    torch_iters = max(3, 640 // horizon)
    res = rounds(fns, {k: 200 if k.startswith("hip") else torch_iters for k in fns})
    for kind in ("norm", "raw"):
        a, b = res[f"torch_{kind}_a"][1], res[f"torch_{kind}_b"][1]
        res[f"{kind}_noise_us"] = round(abs(a - b), 2)
        res[f"{kind}_speedup"] = round(min(a, b) / res[f"hip_{kind}"][1], 1)
        res[f"{kind}_beats_torch_by_more_than_noise"] = bool(res[f"hip_{kind}"][1] + abs(a - b) < min(a, b))
    res.update(envs=envs, agents=4, horizon=horizon, valid_share=round(float(out.valid[slots].float().mean()), 4), agrees=agrees)
    env.close()
    return res


def ppo_iteration(dev, envs=4096, agents=4, rollout=32, iterations=5):
    """Median over `iterations` iterations of the four phases of examples/train_ppo.py's loop, in µs."""
    torch.manual_seed(0)
    venv = UAVVectorEnv(envs, num_agents=agents, device=dev, seed=0)
    mem = DeviceReplay(venv.env, horizon=rollout)
    mem.begin(venv.reset())
    gen = torch.Generator(device=dev).manual_seed(0)
    ppo = PPO(mem, generator=gen)
    ref = TorchGAE(mem, True)
    phases = {k: [] for k in ("acting", "stepping", "update_total", "advantages", "advantages_torch_loop")}

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
        marks["update_total"].append(timed(ppo.update))
        marks["advantages"].append(timed(lambda: ppo.advantages.compute(ppo.values)))
        marks["advantages_torch_loop"].append(timed(lambda: ref(ppo.values, rollout)))
        torch.cuda.synchronize()
        if it:                                        # the first iteration warms everything up
            for k, v in marks.items():
                phases[k].append(sum(a.elapsed_time(b) for a, b in v) * 1e3)
    med = {k: round(sorted(v)[len(v) // 2], 1) for k, v in phases.items()}
    med["torch_update"] = round(med["update_total"] - med["advantages"], 1)
    med["iteration"] = round(med["acting"] + med["stepping"] + med["update_total"], 1)
    med.update(envs=envs, agents=agents, rollout=rollout, epochs=ppo.epochs, minibatches=ppo.minibatches,
               rows=envs * agents * rollout)
    venv.close()
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gae_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(unit="us per call: [min, median, max] of 3 alternating rounds; eager calls, host launch cost included",
               gamma=GAMMA, lam=LAM, gae_sha=_gae_lib.source_hash(), device=torch.cuda.get_device_name(0),
               rings=[measure(envs, horizon, dev) for envs, horizon in RINGS], ppo_iteration_us=ppo_iteration(dev))
    text = json.dumps(res, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

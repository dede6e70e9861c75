#!/usr/bin/env python3
"""Times prioritized n-step replay (libuavx_keywalk.so) on the trainers' ring -- 1024 envs x 4 agents, horizon
256, stepped past the wrap with step_cap = 1500, the ring and the method of tools/prio_bench.py -- as graph-captured calls:

  parent_a, parent_b   PrioritizedReplaySampler.sample (§23), captured and timed TWICE: the larger relative gap between the
                       two, over the rounds and over their medians, is the noise margin of this run
  per_nstep_N          PrioritizedNStepSampler.sample at n_step = N: the parent's launches and the walk launch
  walk_N               the walk launch alone (KeyWalk.extend on the keys of a sample)
  nstep_N              NStepReplaySampler.sample at n_step = N (§22): what a walk costs next to a uniform draw
  update               a captured FusedSAC / FusedDDPG update with prioritized=0.6, per_beta=0.4 at per_n_step 1 and 3

The variants are timed in turn, three rounds of them, so that a drift of the machine hits all alike; every figure is the
median over the rounds of critic_bench.time_us (itself the median of three timed loops), with [min, max] beside it.  One JSON
line per batch size and one per learner, carrying the libraries' hashes; --out also writes them into one JSON file.

    python tools/prio_nstep_bench.py [--rows 256 262144] [--iters 200] [--out profiles/prio_nstep_bench.json]
"""
import argparse
import datetime
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from critic_bench import time_us                                                        # noqa: E402
from prio_bench import graphed, ring                                                    # noqa: E402
from gym_uav_collision_avoidance_amd import _keywalk_lib, _prio_lib, learners           # noqa: E402
from gym_uav_collision_avoidance_amd.fused_replay_nstep import NStepReplaySampler      # noqa: E402
from gym_uav_collision_avoidance_amd.prioritized_nstep import KeyWalk, PrioritizedNStepSampler       # noqa: E402
from gym_uav_collision_avoidance_amd.prioritized_replay import PrioritizedReplaySampler  # noqa: E402

STEPS = (1, 3, 5, 8)


def rounds(replays, iters, n=3):
    """{name: [per-round us]} of the replays taking turns, n rounds."""
    ts = {k: [] for k in replays}
    for _ in range(n):
        for k, fn in replays.items():
            ts[k].append(time_us(fn, iters))
    return ts


def summary(ts):
    return {k: dict(us=round(sorted(v)[len(v) // 2], 2), min_max=[round(min(v), 2), round(max(v), 2)]) for k, v in ts.items()}


def spread(per, rows, gen, dev):
    """Priorities as a run of updates leaves them, so that the search and the weights do real work."""
    batch = per.sample(rows, generator=gen)
    per.update_priorities(batch[6], torch.rand(rows, generator=gen, device=dev) * 4)
    return per.sample(rows, generator=gen)


def samplers(mem, rows, iters, dev):
    gen = torch.Generator(device=dev).manual_seed(2)
    fns, keep = {}, []
    for name in ("parent_a", "parent_b"):
        per = PrioritizedReplaySampler(mem, alpha=0.6, beta=0.4).reserve(rows)
        spread(per, rows, gen, dev)
        outs = per._outputs(rows, False, None)
        fns[name] = (lambda per=per, outs=outs: per.sample(rows, generator=gen, out=outs), gen)
    for n in STEPS:
        per = PrioritizedNStepSampler(mem, alpha=0.6, beta=0.4, n_step=n, gamma=0.99).reserve(rows)
        batch = spread(per, rows, gen, dev)
        outs = tuple(torch.empty_like(t) for t in batch)
        fns[f"per_nstep_{n}"] = (lambda per=per, outs=outs: per.sample(rows, generator=gen, out=outs), gen)
        walk = KeyWalk(mem, n_step=n, gamma=0.99)
        key, r, s2, m = batch[6].clone(), batch[2].clone(), batch[3].clone(), batch[4].clone()
        fns[f"walk_{n}"] = (lambda walk=walk, a=(key, r, s2, m): walk.extend(*a), None)
        uni = NStepReplaySampler(mem, n_step=n, gamma=0.99).reserve(rows)
        uouts = tuple(torch.empty_like(t) for t in uni.sample(rows, generator=gen))
        fns[f"nstep_{n}"] = (lambda uni=uni, uouts=uouts: uni.sample(rows, generator=gen, out=uouts), gen)
        keep += [per, walk, uni]
    graphs = {name: graphed(fn, g) for name, (fn, g) in fns.items()}
    ts = rounds({name: g.replay for name, g in graphs.items()}, iters)
    res = summary(ts)
    a, b = ts["parent_a"], ts["parent_b"]
    gaps = [abs(x - y) / min(x, y) for x, y in zip(a, b)] + [abs(res["parent_a"]["us"] - res["parent_b"]["us"])
                                                             / min(res["parent_a"]["us"], res["parent_b"]["us"])]
    parent = (res["parent_a"]["us"] + res["parent_b"]["us"]) / 2
    res["noise_margin"] = round(max(gaps), 4)
    res["parent_us"] = round(parent, 2)
    for n in STEPS:
        res[f"per_nstep_{n}_minus_parent_us"] = round(res[f"per_nstep_{n}"]["us"] - parent, 2)
    res["n_step_1_over_parent_beyond_margin_us"] = round(max(0.0, res["per_nstep_1"]["us"] - parent * (1 + max(gaps))), 2)
    del graphs
    return res


class Update:
    def __init__(self, kind, mem, rows, per_n_step, dev):
        torch.manual_seed(0)
        cls = {"sac": learners.FusedSAC, "ddpg": learners.FusedDDPG}[kind]
        self.agent = cls(device=dev, memory=mem, prioritized=0.6, per_beta=0.4, per_n_step=per_n_step)
        self.agent.capture(rows)

    def replay(self):
        self.agent.run(1)


def updates(mem, rows, iters, dev):
    out = []
    for kind in ("sac", "ddpg"):
        arms = {f"per_n_step_{n}": Update(kind, mem, rows, n, dev) for n in (1, 3)}
        res = summary(rounds({k: v.replay for k, v in arms.items()}, iters))
        res["per_n_step_3_minus_1_us"] = round(res["per_n_step_3"]["us"] - res["per_n_step_1"]["us"], 2)
        res["finite"] = all(bool(torch.isfinite(torch.from_numpy(v.agent.losses(last=1))).all()) for v in arms.values())
        out.append(dict(learner=kind, rows=rows, iters=iters, prioritized=0.6, per_beta=0.4, **res))
        for v in arms.values():
            v.agent.close()
        del arms
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 262144])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--update-rows", type=int, default=256)
    ap.add_argument("--update-iters", type=int, default=30)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=256)
    ap.add_argument("--step-cap", type=int, default=1500)
    ap.add_argument("--out", default=None, help="also write every line into this JSON file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    env, mem = ring(a.envs, a.horizon, a.step_cap, dev)
    head = dict(tool="tools/prio_nstep_bench.py", date=datetime.date.today().isoformat(),
                device=torch.cuda.get_device_name(0), keywalk_sha=_keywalk_lib.source_hash(), prio_sha=_prio_lib.source_hash(),
                envs=a.envs, agents=4, horizon=a.horizon, steps=mem.count, step_cap=a.step_cap)
    lines = []
    for rows in a.rows:
        lines.append(dict(rows=rows, iters=a.iters, **samplers(mem, rows, a.iters, dev)))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    for line in updates(mem, a.update_rows, a.update_iters, dev):
        lines.append(line)
        print(json.dumps(line), flush=True)
    env.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(head, results=lines), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

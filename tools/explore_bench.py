#!/usr/bin/env python3
"""Times the graph-captured acting step two ways in one process: the exploration launch behind the RAW forward
(exploration.py) and the acting step as it had to be written before --
    SAC, TD3   FusedActor.act(evaluate=False): torch.randn + one forward with the noise in its epilogue
    DDPG       the Ornstein-Uhlenbeck recurrence of ou.py in torch element-wise ops on a float64 [rows, 1] tensor, then
               FusedActor.act(evaluate=False, noise=x)
Both write the same [rows, 2] action buffer.  The two take turns three times (median, min, max of 30 replays each).  One
JSON line per (learner, rows), carrying the library's actor_sha.

    python tools/explore_bench.py [--rows 4096 262144] [--iters 30] [--out profiles/r16_explore_bench.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from action_grad_bench import alternated                                          # noqa: E402
from critic_grad_bench import graphed                                             # noqa: E402
from gym_uav_collision_avoidance_amd import _actor_lib, policy                    # noqa: E402
from gym_uav_collision_avoidance_amd.exploration import Exploration               # noqa: E402
from gym_uav_collision_avoidance_amd.fused_actor import FusedActor                # noqa: E402

ACTORS = {"sac": policy.GaussianPolicy, "td3": policy.TD3Actor, "ddpg": policy.DDPGActor}
SIGMA, THETA, DT, MEAN = 0.2, 0.15, 1e-2, 0.0


def old_step(kind, fa, obs, out, x, z):
    if kind != "ddpg":
        return lambda: fa.act(obs, evaluate=False, out=out)
    s = SIGMA * DT ** 0.5

    def step():
        x.add_(THETA * (MEAN - x) * DT + s * z.normal_())                        # ou.py:18-22 on every row's own value
        fa.act(obs, evaluate=False, noise=x, out=out)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 262144])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--learners", nargs="+", default=list(ACTORS))
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sha = _actor_lib.source_hash()
    for rows in a.rows:
        obs = torch.rand((rows, 10), generator=torch.Generator(device=dev).manual_seed(0), device=dev) * 2 - 1
        for kind in a.learners:
            torch.manual_seed(0)
            fa = FusedActor.from_module(ACTORS[kind]().to(dev).eval())
            ex = Exploration(fa, rows, seed=1, ou_sigma=SIGMA, ou_theta=THETA, ou_dt=DT, ou_mean=MEAN)
            out_new, out_old = (torch.empty((rows, 2), device=dev) for _ in range(2))
            x, z = (torch.zeros((rows, 1), dtype=torch.float64, device=dev) for _ in range(2))
            graphs = dict(act_new_graph_us=graphed(lambda: ex.act(obs, out=out_new)),
                          act_old_graph_us=graphed(old_step(kind, fa, obs, out_old, x, z)))
            res = dict(learner=kind, rows=rows, actor_sha=sha, iters=a.iters)
            for k, v in alternated(graphs, a.iters).items():
                res[k], res[k + "_min_max"] = v[0], v[1:]
            res["new_minus_old_us"] = res["act_new_graph_us"] - res["act_old_graph_us"]
            res["new_vs_old"] = res["act_new_graph_us"] / res["act_old_graph_us"]
            res["finite"] = bool(torch.isfinite(out_new).all() and torch.isfinite(out_old).all()
                                 and float(out_new.abs().max()) <= 1.0)
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            fa.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

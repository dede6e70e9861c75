#!/usr/bin/env python3
"""Times the fused critic action-gradient (FusedActionGrad.q_dqda, one launch) of each learner beside torch's critic part of
the actor update (critic forward + autograd.grad with respect to the action, the towers the learner's loss uses) run
eagerly in f32 and captured in a CUDA graph, and the whole actor-loss block both ways, both graph-captured: torch =
`zero_grad(); loss.backward()` of sac.py:70-78 / td3.py:144 / ddpg.py:77-79 on the modules; fused =
FusedActorLoss.backward.  The graph timings are alternated three times (median, min, max).  One JSON line per
(learner, rows), carrying the library's actor_sha.  torch is the baseline, measured in the same run.

    python tools/action_grad_bench.py [--rows 256 4096 65536] [--iters 30] [--out profiles/r13_action_grad_bench.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from critic_bench import PAIRS, time_us                                           # noqa: E402
from critic_grad_bench import graphed                                             # noqa: E402
from gym_uav_collision_avoidance_amd import _actor_lib                            # noqa: E402
from gym_uav_collision_avoidance_amd.fused_critic import FusedActionGrad, FusedActorLoss   # noqa: E402


def alternated(graphs, iters, rounds=3):
    """{name: (median, min, max) us} of graph replays, the graphs taking turns."""
    ts = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, gr in graphs.items():
            ts[k].append(time_us(gr.replay, iters))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 4096, 65536])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--learners", nargs="+", default=list(PAIRS))
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sha = _actor_lib.source_hash()
    for rows in a.rows:
        g = torch.Generator(device=dev).manual_seed(0)
        s = torch.randn((rows, 10), generator=g, device=dev)
        act = torch.rand((rows, 2), generator=g, device=dev) * 2 - 1
        eps = torch.randn((rows, 2), generator=g, device=dev)
        alpha = torch.tensor([0.2], device=dev)
        for name in a.learners:
            acls, ccls = PAIRS[name]
            torch.manual_seed(0)
            actor, critic = acls().to(dev), ccls().to(dev)
            mask = 1 if name == "td3" else None
            act_g = act.clone().requires_grad_(True)

            def torch_jac():
                out = critic(s, act_g)
                qs = out if isinstance(out, tuple) else (out,)
                qs = qs[:1] if name == "td3" else qs
                return torch.autograd.grad(sum(q.sum() for q in qs), act_g)

            def torch_block():
                if name == "sac":
                    mean, log_std = actor(s)
                    std = log_std.exp()
                    normal = torch.distributions.Normal(mean, std, validate_args=False)
                    x_t = mean + std * eps
                    y_t = torch.tanh(x_t)
                    lp = (normal.log_prob(x_t) - torch.log(1 * (1 - y_t.pow(2)) + 1e-6)).sum(1, keepdim=True)
                    loss = ((alpha * lp) - torch.min(*critic(s, y_t))).mean()
                elif name == "td3":
                    loss = -critic(s, actor(s))[0].mean()
                else:
                    loss = -critic(s, actor(s)).mean()
                for p in actor.parameters():
                    p.grad = None
                loss.backward()

            ag = FusedActionGrad(critic)
            out = (torch.empty((ag.critic.towers, rows), device=dev), torch.empty((ag.critic.towers, rows, 2), device=dev))
            al = FusedActorLoss(actor, ag)
            fused_jac = lambda: ag.q_dqda(s, act, towers=mask, out=out)
            fused_block = lambda: al.backward(s, alpha=alpha, noise=eps)

            res = dict(learner=name, rows=rows, actor_sha=sha)
            res["launch_fused_us"] = time_us(fused_jac, a.iters)
            res["launch_torch_eager_us"] = time_us(torch_jac, a.iters)
            graphs = dict(launch_fused_graph_us=graphed(fused_jac), launch_torch_graph_us=graphed(torch_jac))
            for k, v in alternated(graphs, a.iters).items():
                res[k], res[k + "_min_max"] = v[0], v[1:]
            del graphs
            res["block_fused_eager_us"] = time_us(fused_block, a.iters)
            res["block_torch_eager_us"] = time_us(torch_block, a.iters)
            graphs = dict(block_fused_graph_us=graphed(fused_block), block_torch_graph_us=graphed(torch_block))
            for k, v in alternated(graphs, a.iters).items():
                res[k], res[k + "_min_max"] = v[0], v[1:]
            del graphs
            for p in critic.parameters():
                p.grad = None
            res.update(launch_ratio_vs_graph=res["launch_fused_graph_us"] / res["launch_torch_graph_us"],
                       block_ratio_vs_graph=res["block_fused_graph_us"] / res["block_torch_graph_us"])
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            al.close()
            ag.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

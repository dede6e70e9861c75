#!/usr/bin/env python3
"""Times the learners' actor-loss block three ways, each captured in a CUDA graph: FusedPolicyGrad.backward (five HIP
launches: actor forward, critic action-gradient, actor backward, weights, combine), FusedActorLoss.backward (the critic in
one launch, the actor under torch autograd; the block before FusedPolicyGrad and the baseline here) and torch's own
`p.grad = None; loss.backward()` of sac.py:70-78 / td3.py:144 / ddpg.py:77-79 on the modules.  The three graphs take turns
three times (median, min, max of 30 replays each).  One JSON line per (learner, rows), carrying the library's actor_sha.

    python tools/policy_grad_bench.py [--rows 256 4096 65536] [--iters 30] [--out profiles/r14_policy_grad_bench.jsonl]
    rocprofv3 --kernel-trace --stats -d out -- python tools/policy_grad_bench.py --rows 256 --only-fused 50
        # the five launches' own times: only the new block runs, eagerly, 50 times per learner
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
from critic_bench import PAIRS, time_us                                           # noqa: E402
from critic_grad_bench import graphed                                             # noqa: E402
from gym_uav_collision_avoidance_amd import _actor_lib                            # noqa: E402
from gym_uav_collision_avoidance_amd.fused_critic import FusedActionGrad, FusedActorLoss   # noqa: E402
from gym_uav_collision_avoidance_amd.fused_policy_grad import FusedPolicyGrad     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 4096, 65536])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--learners", nargs="+", default=list(PAIRS))
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--only-fused", type=int, default=0, metavar="N",
                    help="run only FusedPolicyGrad.backward, eagerly, N times per cell (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sha = _actor_lib.source_hash()
    for rows in a.rows:
        g = torch.Generator(device=dev).manual_seed(0)
        s = torch.randn((rows, 10), generator=g, device=dev)
        eps = torch.randn((rows, 2), generator=g, device=dev)
        alpha = torch.tensor([0.2], device=dev)
        for name in a.learners:
            acls, ccls = PAIRS[name]
            torch.manual_seed(0)
            actor, critic = acls().to(dev), ccls().to(dev)

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
            al = FusedActorLoss(actor, ag)
            pg = FusedPolicyGrad(actor, ag).reserve(rows)
            new_block = lambda: pg.backward(s, alpha=alpha, noise=eps)
            parent_block = lambda: al.backward(s, alpha=alpha, noise=eps)
            if a.only_fused:
                for _ in range(a.only_fused):
                    new_block()
                torch.cuda.synchronize()
                continue

            res = dict(learner=name, rows=rows, actor_sha=sha)
            res["block_new_eager_us"] = time_us(new_block, a.iters)
            res["block_parent_eager_us"] = time_us(parent_block, a.iters)
            res["block_torch_eager_us"] = time_us(torch_block, a.iters)
            graphs = dict(block_torch_graph_us=graphed(torch_block), block_parent_graph_us=graphed(parent_block))
            for p in actor.parameters():
                p.grad = None                          # the new block then writes its own buffers, not a graph pool's
            graphs["block_new_graph_us"] = graphed(new_block)
            for k, v in alternated(graphs, a.iters).items():
                res[k], res[k + "_min_max"] = v[0], v[1:]
            del graphs
            for p in critic.parameters():
                p.grad = None
            res.update(new_vs_parent=res["block_new_graph_us"] / res["block_parent_graph_us"],
                       new_vs_torch=res["block_new_graph_us"] / res["block_torch_graph_us"])
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

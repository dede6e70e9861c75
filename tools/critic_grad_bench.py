#!/usr/bin/env python3
"""Times the fused critic-loss gradient (FusedCriticLoss.backward, three launches) of each learner beside torch's block
(forward + loss + zero_grad + backward, sac.py:61-68, td3.py:129-138, ddpg.py:63-71) run eagerly in f32 and captured in a
CUDA graph, and the whole critic update both ways: torch = target (no-grad) + that block + Adam step; fused = FusedTarget +
FusedCriticLoss + the same Adam step (eager and graph-captured).  One JSON line per (learner, rows), carrying the
library's actor_sha.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/critic_grad_bench.py` for the
per-kernel summary.

    python tools/critic_grad_bench.py [--rows 256 4096 65536 262144] [--iters 30]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from critic_bench import PAIRS, time_us, torch_block                             # noqa: E402
from gym_uav_collision_avoidance_amd import _actor_lib                           # noqa: E402
from gym_uav_collision_avoidance_amd.fused_critic import FusedCriticLoss, FusedTarget   # noqa: E402


def graphed(fn):
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        fn()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 4096, 65536, 262144])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--learners", nargs="+", default=list(PAIRS))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sha = _actor_lib.source_hash()
    for rows in a.rows:
        g = torch.Generator(device=dev).manual_seed(0)
        s = torch.randn((rows, 10), generator=g, device=dev)
        act = torch.rand((rows, 2), generator=g, device=dev) * 2 - 1
        s2 = torch.randn((rows, 10), generator=g, device=dev)
        r = torch.randn((rows, 1), generator=g, device=dev)
        m = (torch.rand((rows, 1), generator=g, device=dev) > 0.05).float()
        eps = torch.randn((rows, 2), generator=g, device=dev)
        y = torch.randn((rows, 1), generator=g, device=dev)
        alpha = torch.tensor([0.2], device=dev)
        yout = torch.empty((rows, 1), device=dev)
        for name in a.learners:
            acls, ccls = PAIRS[name]
            torch.manual_seed(0)
            actor, critic, target = acls().to(dev), ccls().to(dev), ccls().to(dev)
            opt = torch.optim.Adam(critic.parameters(), lr=3e-4, amsgrad=name == "ddpg", capturable=True)

            def torch_grad(yy=y):
                out = critic(s, act)
                qs = out if isinstance(out, tuple) else (out,)
                loss = sum(F.mse_loss(q, yy) for q in qs) if name != "ddpg" else F.l1_loss(yy, qs[0])
                opt.zero_grad(set_to_none=False)
                loss.backward()

            def torch_update():
                torch_grad(torch_block(name, actor, target, s2, r, m, eps, alpha))
                opt.step()

            closs = FusedCriticLoss(critic).reserve(rows)
            ft = FusedTarget(actor, target)
            fused_grad = lambda: closs.backward(s, act, y)

            def fused_update():
                closs.backward(s, act, ft(s2, r, m, alpha=alpha, noise=eps, out=yout))
                opt.step()

            res = dict(learner=name, rows=rows, actor_sha=sha)
            res["fused_us"] = time_us(fused_grad, a.iters)
            res["torch_eager_us"] = time_us(torch_grad, a.iters)
            gr = graphed(torch_grad)
            res["torch_graph_us"] = time_us(gr.replay, a.iters)
            del gr
            res["update_fused_us"] = time_us(fused_update, a.iters)
            gr = graphed(fused_update)
            res["update_fused_graph_us"] = time_us(gr.replay, a.iters)
            del gr
            res["update_torch_eager_us"] = time_us(torch_update, a.iters)
            gr = graphed(torch_update)
            res["update_torch_graph_us"] = time_us(gr.replay, a.iters)
            del gr
            res.update(speedup_vs_eager=res["torch_eager_us"] / res["fused_us"],
                       ratio_vs_graph=res["fused_us"] / res["torch_graph_us"],
                       update_ratio_vs_graph=res["update_fused_graph_us"] / res["update_torch_graph_us"],
                       workspace_mib=closs.workspace_bytes(rows) / 2**20)
            print(json.dumps(res), flush=True)
            ft.close()
            closs.close()
            del closs, opt
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

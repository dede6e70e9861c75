#!/usr/bin/env python3
"""Times the fused TD target (FusedTarget, one launch) of each learner in f32 and bf16 beside torch's no-grad block
(sac.py:56-60, td3.py:114-127, ddpg.py:62) run eagerly in f32 and the same block captured in a CUDA graph; one JSON line
per (learner, precision, rows).  The fused target is timed with the default small-batch threshold and with each variant
forced (fused_small_us / fused_large_us), which is how UAVX_CRITIC_SPLIT_ROWS was chosen.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/critic_bench.py` for the per-kernel summary.

    python tools/critic_bench.py [--rows 256 4096 65536 262144] [--iters 50]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_uav_collision_avoidance_amd import _actor_lib, policy                 # noqa: E402
from gym_uav_collision_avoidance_amd.fused_critic import FusedTarget            # noqa: E402

PAIRS = {"sac": (policy.GaussianPolicy, policy.TwinQ), "td3": (policy.TD3Actor, policy.TD3TwinQ),
         "ddpg": (policy.DDPGActor, policy.DDPGCritic)}


def time_us(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / iters)
    return sorted(ts)[1]


def torch_block(name, actor, critic, s2, r, m, eps, alpha, gamma=0.99):
    with torch.no_grad():
        if name == "sac":
            mean, log_std = actor(s2)
            std = log_std.exp()
            normal = torch.distributions.Normal(mean, std, validate_args=False)
            x_t = normal.loc + eps * normal.scale
            y_t = torch.tanh(x_t)
            lp = (normal.log_prob(x_t) - torch.log(1 * (1 - y_t.pow(2)) + 1e-6)).sum(1, keepdim=True)
            q1, q2 = critic(s2, y_t)
            return r + m * gamma * (torch.min(q1, q2) - alpha * lp)
        if name == "td3":
            a = (actor(s2) + (eps * 0.2).clamp(-0.5, 0.5)).clamp(-1, 1)
            return r + m * gamma * torch.min(*critic(s2, a))
        return r + gamma * m * critic(s2, actor(s2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 4096, 65536, 262144])
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for rows in a.rows:
        g = torch.Generator(device=dev).manual_seed(0)
        s2 = torch.randn((rows, 10), generator=g, device=dev)
        r = torch.randn((rows, 1), generator=g, device=dev)
        m = (torch.rand((rows, 1), generator=g, device=dev) > 0.05).float()
        eps = torch.randn((rows, 2), generator=g, device=dev)
        alpha = torch.tensor([0.2], device=dev)
        out = torch.empty((rows, 1), device=dev)
        for name, (acls, ccls) in PAIRS.items():
            torch.manual_seed(0)
            actor, critic = acls().to(dev).eval(), ccls().to(dev).eval()
            blk = lambda: torch_block(name, actor, critic, s2, r, m, eps, alpha)
            t_eager = time_us(blk, a.iters)
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                blk()
            torch.cuda.current_stream().wait_stream(side)
            with torch.cuda.graph(graph):
                blk()
            t_graph = time_us(graph.replay, a.iters)
            del graph
            for prec in ("f32", "bf16"):
                ft = FusedTarget(actor, critic, precision=prec)
                call = lambda: ft(s2, r, m, alpha=alpha, noise=eps, out=out)
                res = dict(learner=name, precision=prec, rows=rows, fused_us=time_us(call, a.iters))
                ft.set_split_rows(1 << 62)
                res["fused_small_us"] = time_us(call, a.iters)
                ft.set_split_rows(0)
                res["fused_large_us"] = time_us(call, a.iters)
                ft.set_split_rows(_actor_lib.SPLIT_ROWS)
                res.update(torch_eager_f32_us=t_eager, torch_graph_f32_us=t_graph,
                           speedup_vs_eager=t_eager / res["fused_us"], ratio_vs_graph=res["fused_us"] / t_graph)
                print(json.dumps(res), flush=True)
                ft.close()


if __name__ == "__main__":
    main()

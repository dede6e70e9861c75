#!/usr/bin/env python3
"""Times the fused actor kernel (FusedActor.act, DETERMINISTIC) of each policy.py actor in f32 and bf16 at 262 144 and
524 288 rows, beside the torch module's act() on the same rows; one JSON line per case.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/actor_bench.py` for the per-kernel summary.

    python tools/actor_bench.py [--rows 262144 524288] [--iters 50]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_uav_collision_avoidance_amd.fused_actor import FusedActor                  # noqa: E402
from gym_uav_collision_avoidance_amd.policy import DDPGActor, GaussianPolicy, TD3Actor   # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[262144, 524288])
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for rows in a.rows:
        x = torch.rand((rows, 10), device=dev)
        out = torch.empty((rows, 2), device=dev)
        for cls in (GaussianPolicy, TD3Actor, DDPGActor):
            torch.manual_seed(0)
            pol = cls().to(dev).eval()
            res = dict(actor=cls.__name__, rows=rows, torch_f32_us=time_us(lambda: pol.act(x), a.iters))
            pb, xb = pol.to(torch.bfloat16), x.to(torch.bfloat16)
            res["torch_bf16_us"] = time_us(lambda: pb.act(xb), a.iters)
            pol = pol.float()
            for prec in ("f32", "bf16"):
                fa = FusedActor.from_module(pol, precision=prec)
                res[f"fused_{prec}_us"] = time_us(lambda: fa.act(x, out=out), a.iters)
                fa.close()
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

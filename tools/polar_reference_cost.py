#!/usr/bin/env python3
"""Launches of uavx_step_ex with polar=True and with polar="reference" on float32 policy outputs, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/polar_reference_cost.py [--shape 65536x4 | 65536x8 | cfg5]

cfg5 is bench.py --cfg5's world (65 536 envs x 8 UAVs + 16 scripted bodies, 4-level curriculum).  Each mode runs --iters
launches after a warm-up, fed from a ring of distinct action batches; auto-reset on agent 0's done with a 1 500-step cap,
episode returns tracked (the closed loop's options).  step_ex_kernel rows are polar=True, step_ex_ref_kernel rows are
polar="reference"; the mean launch time of each is in the trace's kernel statistics.  Prints host-timed us per launch too."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="65536x4", choices=("65536x4", "65536x8", "cfg5"))
ap.add_argument("--iters", type=int, default=400)
args = ap.parse_args()
if args.shape == "cfg5":
    env = BatchedMultiUAVWorld2D(65536, num_agents=8, num_bodies=16, seed=1)
    f = lambda a, b, k: a + (b - a) * k / 3
    env.set_curriculum([dict(x_size=f(30.0, 60.0, k), y_size=f(30.0, 60.0, k), collider_radius=1.0, d_sense=f(10.0, 18.0, k),
                             n_active=max(1, round(f(4, 8, k))), b_active=round(f(4, 16, k))) for k in range(4)], lo=0, hi=3)
else:
    E, N = (int(x) for x in args.shape.split("x"))
    env = BatchedMultiUAVWorld2D(E, num_agents=N, seed=1)
env.reset()
g = torch.Generator(device=env.device).manual_seed(0)
ring = [torch.rand((env.num_envs, env.num_agents, 2), generator=g, device=env.device) * 2 - 1 for _ in range(16)]
out = {}
for polar in (True, "reference", True, "reference"):   # twice each, interleaved: the second pair is the one reported
    kw = dict(polar=polar, auto_reset="agent0_done", step_cap=1500, track_returns=True)
    for i in range(50):
        env.step_ex(ring[i % 16], **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.iters):
        env.step_ex(ring[i % 16], **kw)
    torch.cuda.synchronize()
    out[str(polar)] = (time.perf_counter() - t0) / args.iters * 1e6
print(json.dumps(dict(shape=args.shape, host_us_per_launch=out)))
env.close()

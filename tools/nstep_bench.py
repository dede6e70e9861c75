#!/usr/bin/env python3
"""Times one graph-captured sample of NStepReplaySampler (libuavx_actor.so) beside FusedReplaySampler's
(§16) on the same ring in the same process: 1024 envs x 4 agents, horizon 256, stepped past the wrap with step_cap = 1500.

Per batch size, in this order: the one-step baseline twice, back to back (the larger relative difference of the two is
the noise margin), n_step = 1 / recency = 0 (the same kernels through the same launch path as the baseline: a third
timing of it, reported against that margin), then n_step 3, 5, 8 with recency 0.8, which have no bound.  Every figure is
the median of three time_us() runs of graph replays (critic_bench.time_us: itself the median of three timed loops).  One
JSON line per batch size, carrying the library's actor_sha.

    python tools/nstep_bench.py [--rows 256 262144] [--iters 200]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from critic_bench import time_us                                                        # noqa: E402
from replay_bench import graphed                                                        # noqa: E402
from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D, _actor_lib           # noqa: E402
from gym_uav_collision_avoidance_amd.fused_replay import FusedReplaySampler            # noqa: E402
from gym_uav_collision_avoidance_amd.fused_replay_nstep import NStepReplaySampler      # noqa: E402
from gym_uav_collision_avoidance_amd.replay import DeviceReplay                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 262144])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=256)
    ap.add_argument("--step-cap", type=int, default=1500)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    env = BatchedMultiUAVWorld2D(a.envs, num_agents=4, device=dev, seed=0)
    mem = DeviceReplay(env, horizon=a.horizon)
    mem.begin(env.reset())
    g = torch.Generator(device=dev).manual_seed(0)
    for _ in range(a.horizon + 16):
        mem.action_slot().copy_(torch.rand((a.envs, 4, 2), generator=g, device=dev) * 2 - 1)
        mem.step(polar=True, auto_reset="agent0_done", step_cap=a.step_cap)
    skip_share = float((mem.skip != 0).float().mean())

    def timed(sampler, rows):
        """Median, min, max of three timings of the captured sample, and the mean length of its rows (None: one step)."""
        sampler.reserve(rows)
        gen = torch.Generator(device=dev).manual_seed(2)
        graph = graphed(lambda: sampler.sample(rows, generator=gen), gen)
        ts = sorted(time_us(graph.replay, a.iters) for _ in range(3))
        length = None
        if isinstance(sampler, NStepReplaySampler):
            length = float(sampler.sample(rows, generator=gen, with_length=True)[5].float().mean())
        del graph
        return ts, length

    for rows in a.rows:
        one = FusedReplaySampler(mem)
        same = NStepReplaySampler(mem, n_step=1, gamma=0.99, recency=0.0)
        g1, g2 = torch.Generator(device=dev).manual_seed(1), torch.Generator(device=dev).manual_seed(1)
        if not all(torch.equal(x, y) for x, y in zip(one.sample(rows, generator=g1, with_flags=True),
                                                     same.sample(rows, generator=g2, with_flags=True))):
            raise SystemExit(f"nstep_bench: n_step = 1 and the one-step sampler differ at {rows} rows")
        res = dict(rows=rows, actor_sha=_actor_lib.source_hash(), envs=a.envs, agents=4, horizon=a.horizon,
                   steps=mem.count, step_cap=a.step_cap, reset_row_share=skip_share, iters=a.iters)
        (base_a, _), (base_b, _) = timed(one, rows), timed(one, rows)
        res.update(baseline_us=[base_a[1], base_b[1]], baseline_min_max_us=[base_a[0], base_a[2], base_b[0], base_b[2]])
        margin = abs(base_a[1] - base_b[1]) / min(base_a[1], base_b[1])
        t, _ = timed(same, rows)
        res.update(noise_margin=margin, nstep1_us=t[1], nstep1_min_max_us=[t[0], t[2]],
                   nstep1_vs_baseline=t[1] / min(base_a[1], base_b[1]),
                   nstep1_within_margin=bool(t[1] <= min(base_a[1], base_b[1]) * (1.0 + margin)))
        for n in (3, 5, 8):
            t, length = timed(NStepReplaySampler(mem, n_step=n, gamma=0.99, recency=0.8), rows)
            res[f"nstep{n}_recency08_us"] = t[1]
            res[f"nstep{n}_recency08_min_max_us"] = [t[0], t[2]]
            res[f"nstep{n}_mean_length"] = length
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()
    env.close()


if __name__ == "__main__":
    main()

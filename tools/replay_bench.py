#!/usr/bin/env python3
"""Times the line that opens every learner update, `s, a, r, s2, m = mem.sample(B)`: DeviceReplay.sample (about forty torch
launches) against FusedReplaySampler.sample (two torch.rand + one HIP launch, two above 1024 rows) on the same
ring in the same process -- 4096 envs x 4 agents, horizon 64, stepped past the wrap with a step cap so that reset rows exist.
Both eager and captured in a CUDA graph, alternated, three repeats each (median, min and max given).  The two are first
checked to return the same batch.  One JSON line per batch size, carrying the library's actor_sha.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/replay_bench.py --rows 256 --iters 20` for the launches per sample.

    python tools/replay_bench.py [--rows 256 262144] [--iters 200]
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
from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D, _actor_lib      # noqa: E402
from gym_uav_collision_avoidance_amd.fused_replay import FusedReplaySampler        # noqa: E402
from gym_uav_collision_avoidance_amd.replay import DeviceReplay                     # noqa: E402


def graphed(fn, gen):
    graph = torch.cuda.CUDAGraph()
    graph.register_generator_state(gen)
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
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 262144])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--step-cap", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sha = _actor_lib.source_hash()
    env = BatchedMultiUAVWorld2D(a.envs, num_agents=4, device=dev, seed=0)
    mem = DeviceReplay(env, horizon=a.horizon)
    mem.begin(env.reset())
    g = torch.Generator(device=dev).manual_seed(0)
    for _ in range(a.horizon + 16):
        mem.action_slot().copy_(torch.rand((a.envs, 4, 2), generator=g, device=dev) * 2 - 1)
        mem.step(polar=True, auto_reset="agent0_done", step_cap=a.step_cap)
    sampler = FusedReplaySampler(mem)
    skip_share = float((mem.skip != 0).float().mean())
    for rows in a.rows:
        sampler.reserve(rows)
        g1, g2 = torch.Generator(device=dev).manual_seed(1), torch.Generator(device=dev).manual_seed(1)
        same = all(torch.equal(x, y) for x, y in zip(mem.sample(rows, generator=g1, with_flags=True),
                                                     sampler.sample(rows, generator=g2, with_flags=True)))
        if not same:
            raise SystemExit(f"replay_bench: the fused sampler and DeviceReplay.sample differ at {rows} rows")
        gt, gf = torch.Generator(device=dev).manual_seed(2), torch.Generator(device=dev).manual_seed(2)

        def torch_sample():
            return mem.sample(rows, generator=gt)

        def fused_sample():
            return sampler.sample(rows, generator=gf)

        res = dict(rows=rows, actor_sha=sha, envs=a.envs, agents=4, horizon=a.horizon, steps=mem.count,
                   reset_row_share=skip_share, identical=same, iters=a.iters)
        fe, te = [], []
        for _ in range(3):                                   # alternated: the spread of the same measurement
            fe.append(time_us(fused_sample, a.iters))
            te.append(time_us(torch_sample, a.iters))
        res.update(fused_eager_us=sorted(fe)[1], fused_eager_min_us=min(fe), fused_eager_max_us=max(fe),
                   torch_eager_us=sorted(te)[1], torch_eager_min_us=min(te), torch_eager_max_us=max(te))
        graph_f, graph_t = graphed(fused_sample, gf), graphed(torch_sample, gt)
        fs, ts = [], []
        for _ in range(3):
            fs.append(time_us(graph_f.replay, a.iters))
            ts.append(time_us(graph_t.replay, a.iters))
        res.update(fused_graph_us=sorted(fs)[1], fused_graph_min_us=min(fs), fused_graph_max_us=max(fs),
                   torch_graph_us=sorted(ts)[1], torch_graph_min_us=min(ts), torch_graph_max_us=max(ts))
        res.update(ratio_vs_eager=res["fused_eager_us"] / res["torch_eager_us"],
                   ratio_vs_graph=res["fused_graph_us"] / res["torch_graph_us"], ratio_vs_graph_worst=max(fs) / min(ts))
        print(json.dumps(res), flush=True)
        del graph_f, graph_t
        torch.cuda.empty_cache()
    env.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the weighted critic-loss gradient (uavx_wcritic_grad) beside the unweighted one it shares its row
pass with, and a prioritized learner's update with and without the weighted loss, all graph-captured:

  (a) FusedCriticLoss.backward(s, a, y, weight=w, q_out=q) against backward(s, a, y), per learner and batch size.  The
      unweighted baseline is timed twice (base_a, base_b): the spread between the two is the noise margin a difference has
      to exceed.  The weighted call is also timed with the weight alone and with q_out alone.
  (b) one captured update of a learner built with prioritized=0.6, per_beta=0.4 (weighted loss, q from the gradient's row
      pass) against the same learner with per_beta=0 (unweighted loss and the extra q_dqda launch), on a small ring.

The variants are timed in turn, three rounds of them, so that a drift of the machine hits all alike; every figure is
[min, median, max] over the rounds of critic_bench.time_us (itself the median of three timed loops).  One JSON line per
measurement, carrying the library's actor_sha; all of them also go to profiles/wgrad_bench.json.

    python tools/wgrad_bench.py [--rows 256 262144] [--kinds sac ddpg] [--iters 200] [--update-rows 256]
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
from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D, _actor_lib, learners, policy  # noqa: E402
from gym_uav_collision_avoidance_amd.fused_critic import FusedCriticLoss                # noqa: E402
from gym_uav_collision_avoidance_amd.replay import DeviceReplay                         # noqa: E402

CRITICS = {"sac": policy.TwinQ, "td3": policy.TD3TwinQ, "ddpg": policy.DDPGCritic}
LEARNERS = {"sac": learners.FusedSAC, "td3": learners.FusedTD3, "ddpg": learners.FusedDDPG}


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


def rounds(fns, iters):
    """{name: [min, median, max]} of three alternating rounds."""
    times = {name: [] for name in fns}
    for _ in range(3):
        for name, fn in fns.items():
            times[name].append(time_us(fn, iters))
    return {k: [round(x, 2) for x in sorted(v)] for k, v in times.items()}


def gradient(kind, rows, iters, dev):
    torch.manual_seed(0)
    m = CRITICS[kind]().to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    s = torch.randn((rows, 10), generator=g, device=dev)
    a = torch.rand((rows, 2), generator=g, device=dev) * 2 - 1
    y = torch.randn((rows, 1), generator=g, device=dev)
    w = torch.rand((rows,), generator=g, device=dev) * 0.95 + 0.05
    cl = FusedCriticLoss(m).reserve(rows)
    q = torch.empty((cl.critic.towers, rows), device=dev)
    graphs = {"base_a": graphed(lambda: cl.backward(s, a, y)),
              "weighted_q": graphed(lambda: cl.backward(s, a, y, weight=w, q_out=q)),
              "weight_only": graphed(lambda: cl.backward(s, a, y, weight=w)),      # which of the two additions costs what
              "q_only": graphed(lambda: cl.backward(s, a, y, q_out=q)),
              "base_b": graphed(lambda: cl.backward(s, a, y))}
    res = rounds({k: v.replay for k, v in graphs.items()}, iters)
    base = [res["base_a"][1], res["base_b"][1]]
    out = dict(what="gradient", learner=kind, rows=rows, iters=iters, **{f"{k}_graph_us": v for k, v in res.items()})
    out["noise_us"] = round(abs(base[0] - base[1]), 2)
    out["weighted_minus_base_us"] = round(res["weighted_q"][1] - min(base), 2)
    out["parity"] = bool(res["weighted_q"][1] <= max(base) + out["noise_us"])
    del graphs
    cl.close()
    return out


def update(kind, rows, iters, dev):
    env = BatchedMultiUAVWorld2D(256, num_agents=4, device=dev, seed=0)
    mem = DeviceReplay(env, horizon=64)
    mem.begin(env.reset())
    g = torch.Generator(device=dev).manual_seed(0)
    for _ in range(64 + 8):
        mem.action_slot().copy_(torch.rand((256, 4, 2), generator=g, device=dev) * 2 - 1)
        mem.step(polar=True, auto_reset="agent0_done", step_cap=1500)
    agents = {}
    for name, beta in (("beta0_a", 0.0), ("beta04", 0.4), ("beta0_b", 0.0)):
        torch.manual_seed(0)
        agents[name] = LEARNERS[kind](device=dev, generator=torch.Generator(device=dev).manual_seed(1), memory=mem,
                                      prioritized=0.6, per_beta=beta).capture(rows)
    res = rounds({k: v.run for k, v in agents.items()}, iters)
    base = [res["beta0_a"][1], res["beta0_b"][1]]
    out = dict(what="update", learner=kind, rows=rows, iters=iters, **{f"{k}_graph_us": v for k, v in res.items()})
    out["noise_us"] = round(abs(base[0] - base[1]), 2)
    out["beta04_minus_beta0_us"] = round(res["beta04"][1] - min(base), 2)
    out["not_slower"] = bool(res["beta04"][1] <= max(base) + out["noise_us"])
    for v in agents.values():
        v.close()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 262144])
    ap.add_argument("--kinds", nargs="+", default=["sac", "ddpg"], choices=sorted(CRITICS))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--update-rows", type=int, default=256, help="batch size of the learner updates (0: skip them)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wgrad_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def emit(res):
        res["actor_sha"] = _actor_lib.source_hash()
        lines.append(res)
        print(json.dumps(res), flush=True)

    for kind in a.kinds:
        for rows in a.rows:
            emit(gradient(kind, rows, max(10, a.iters // 10) if rows > 65536 else a.iters, dev))
            torch.cuda.empty_cache()
    if a.update_rows > 0:
        for kind in a.kinds:
            emit(update(kind, a.update_rows, a.iters, dev))
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

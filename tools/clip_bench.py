#!/usr/bin/env python3
"""Times gradient-norm clipping where the learners use it, everything graph-captured, in three alternating
rounds (min / median / max per case):

  tail     what closes a critic update -- optimiser step + soft update of the critic target + re-pack of the target -- on the
           SAC twin-critic and the DDPG critic shapes:
             clip       FusedAdam(max_grad_norm=...).step(update_target=True, refresh=...)      3 launches + the pack
             plain_a/b  the same tail without the keyword, two objects timed alike: their spread is the noise margin
             torch      clip_grad_norm_(foreach=True) + Adam(capturable=True) + the per-parameter soft-update loop + the pack
  update   a captured 256-row learner update (FusedSAC, FusedDDPG: sampling included), with and without max_grad_norm.

Writes profiles/clip_bench.json (one object) and prints it.

    python tools/clip_bench.py [--rows 256] [--iters 200] [--out profiles/clip_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from critic_bench import PAIRS                                                      # noqa: E402
from prio_bench import ring                                                         # noqa: E402
from wgrad_bench import graphed, rounds                                             # noqa: E402
from gym_uav_collision_avoidance_amd import _actor_lib, _clip_lib                   # noqa: E402
from gym_uav_collision_avoidance_amd.fused_critic import FusedCriticLoss, FusedTarget   # noqa: E402
from gym_uav_collision_avoidance_amd.fused_optim import FusedAdam                   # noqa: E402
from gym_uav_collision_avoidance_amd.learners import FusedDDPG, FusedSAC            # noqa: E402

TAU = 5e-3
BOUND = 10.0


def tails(name, rows, iters, dev):
    acls, ccls = PAIRS[name]
    g = torch.Generator(device=dev).manual_seed(0)
    s = torch.randn((rows, 10), generator=g, device=dev)
    act = torch.rand((rows, 2), generator=g, device=dev) * 2 - 1
    s2 = torch.randn((rows, 10), generator=g, device=dev)
    r = torch.randn((rows, 1), generator=g, device=dev)
    m = (torch.rand((rows, 1), generator=g, device=dev) > 0.05).float()
    eps = torch.randn((rows, 2), generator=g, device=dev)
    alpha = torch.tensor([0.2], device=dev)
    torch.manual_seed(0)
    actor, critic, target = acls().to(dev), ccls().to(dev), ccls().to(dev)
    ft = FusedTarget(actor, target)
    closs = FusedCriticLoss(critic).reserve(rows)
    closs.backward(s, act, ft(s2, r, m, alpha=alpha, noise=eps))                     # leaves a gradient in every .grad
    kw = dict(lr=3e-4, amsgrad=name == "ddpg")
    params = list(critic.parameters())
    topt = torch.optim.Adam(params, capturable=True, **kw)
    fused = {k: FusedAdam(torch.optim.Adam(params, **kw), target=target, tau=TAU, **extra)
             for k, extra in (("clip", dict(max_grad_norm=BOUND)), ("plain_a", {}), ("plain_b", {}))}

    def torch_tail():
        torch.nn.utils.clip_grad_norm_(params, BOUND, foreach=True)
        topt.step()
        with torch.no_grad():
            for tp, p in zip(target.parameters(), params):
                tp.data.copy_(tp.data * (1.0 - TAU) + p.data * TAU)
        ft.critic.refresh()

    fns = {k: (lambda o=o: o.step(update_target=True, refresh=ft.critic)) for k, o in fused.items()}
    fns["torch"] = torch_tail
    graphs = {k: graphed(fn) for k, fn in fns.items()}
    res = rounds({k: gr.replay for k, gr in graphs.items()}, iters)
    res.update(tensors=len(params), elements=sum(p.numel() for p in params),
               blocks=sum(-(-p.numel() // _clip_lib.BLOCK) for p in params))
    del graphs
    ft.close()
    closs.close()
    return res


def updates(rows, iters, dev, mem):
    out = {}
    agents = {}
    for name, cls in (("sac", FusedSAC), ("ddpg", FusedDDPG)):
        for k, kw in (("clip", dict(max_grad_norm=BOUND)), ("plain_a", {}), ("plain_b", {})):
            gen = torch.Generator(device=dev).manual_seed(1)
            agents[f"{name}_{k}"] = cls(device=dev, generator=gen, memory=mem, **kw).capture(rows)
    times = rounds({k: (lambda a=a: a.run(1)) for k, a in agents.items()}, iters)
    for k, a in agents.items():
        out[k] = times[k]
        a.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(rows=a.rows, iters=a.iters, bound=BOUND, unit="us per replay: [min, median, max] of 3 alternating rounds",
               actor_sha=_actor_lib.source_hash(), clip_sha=_clip_lib.source_hash(), device=torch.cuda.get_device_name(0),
               tail={name: tails(name, a.rows, a.iters, dev) for name in ("sac", "ddpg")})
    env, mem = ring(1024, 64, 20, dev)
    res["update"] = updates(a.rows, a.iters, dev, mem)
    env.close()
    text = json.dumps(res, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

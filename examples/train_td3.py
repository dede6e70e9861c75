#!/usr/bin/env python3
"""A closed TD3 training loop with nothing leaving the GPU between reports (test_td3_multi.py in batch form): UAVVectorEnv
builds the worlds, DeviceReplay is the ring the step launch writes into, FusedTD3 replays its captured update, and an
Exploration keeps the acting side on the device: uniform random actions while a row is in its warm-up, then the actor's
action plus clipped Gaussian noise drawn from Philox streams keyed by the global agent.

    python examples/train_td3.py [--envs 1024] [--agents 4] [--steps 2000] [--batch 256] [--warmup 64]
                                  [--n-step 1] [--recency 0]       # n-step returns, recency-weighted draws
                                  [--prioritized 0.6]              # proportional prioritized replay
                                  [--per-beta 0.4 --per-beta-final 1.0]   # its weights in the critic loss, annealed (§24)
                                  [--per-n-step 3]                 # n-step returns from its draws (§25)
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_uav_collision_avoidance_amd import UAVVectorEnv
from gym_uav_collision_avoidance_amd.checkpoint import load_run, save_run
from gym_uav_collision_avoidance_amd.learners import FusedTD3
from gym_uav_collision_avoidance_amd.replay import DeviceReplay

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=1024)
ap.add_argument("--agents", type=int, default=4)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--horizon", type=int, default=256)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--warmup", type=int, default=64, help="steps every agent acts uniformly at random for (WARM_UP_STEPS)")
ap.add_argument("--noise-std", type=float, default=0.1, help="standard deviation of the exploration noise")
ap.add_argument("--updates-per-step", type=int, default=1)
ap.add_argument("--report", type=int, default=500)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--checkpoint", type=str, default=None, help="directory to write weights.chpt into at the end")
ap.add_argument("--n-step", type=int, default=1,
                help="steps of return summed per uniformly sampled row (1..8); with --prioritized it is --per-n-step")
ap.add_argument("--recency", type=float, default=0.0, help="share of rows drawn with a weight that grows with recency")
ap.add_argument("--prioritized", type=float, default=None, metavar="ALPHA",
                help="proportional prioritized replay with this exponent (DESIGN.md §23); not with --n-step / --recency: "
                     "its n-step returns are --per-n-step")
ap.add_argument("--per-n-step", type=int, default=1, metavar="N",
                help="steps of return walked from each prioritized draw (1..8, DESIGN.md §25); needs --prioritized")
ap.add_argument("--per-beta", type=float, default=0.0, metavar="B0",
                help="importance-sampling exponent of the prioritized critic loss at the start (DESIGN.md §24); 0: unweighted")
ap.add_argument("--per-beta-final", type=float, default=None, metavar="B1",
                help="anneal the exponent linearly to this value over the run (default: keep B0)")
ap.add_argument("--max-grad-norm", type=float, default=None, metavar="X",
                help="clip the global gradient norm of the critic's and the actor's optimiser step to X (DESIGN.md §26)")
ap.add_argument("--save-run", type=str, default=None, metavar="FILE",
                help="write the whole run (worlds, ring, learner, exploration, generator, step) to FILE at the end (DESIGN.md §27)")
ap.add_argument("--save-every", type=int, default=0, metavar="K", help="also write --save-run's FILE every K env steps")
ap.add_argument("--resume", type=str, default=None, metavar="FILE",
                help="continue the run saved in FILE, built from the same arguments, up to --steps steps in all")
args = ap.parse_args()
if args.per_beta_final is not None and not args.per_beta > 0:
    ap.error("--per-beta-final anneals a weighted loss: give --per-beta B0 > 0 with it")
if args.save_every and not args.save_run:
    ap.error("--save-every writes --save-run's file: give --save-run FILE with it")

dev = torch.device("cuda", 0)
torch.manual_seed(args.seed)           # the networks' initial weights: a run and the same run started again begin alike
venv = UAVVectorEnv(args.envs, num_agents=args.agents, device=dev, seed=args.seed)
mem = DeviceReplay(venv.env, horizon=args.horizon)
mem.begin(venv.reset())
gen = torch.Generator(device=dev).manual_seed(args.seed)
agent = FusedTD3(device=dev, generator=gen, memory=mem, n_step=args.n_step, recency=args.recency,
                 prioritized=args.prioritized, per_beta=args.per_beta, per_n_step=args.per_n_step,
                 max_grad_norm=args.max_grad_norm)
explore = agent.exploration(mem, seed=args.seed, warmup_steps=args.warmup, noise_std=args.noise_std)

run = dict(env=venv.env, memory=mem, agent=agent, exploration=explore, generator=gen)
first = 0                  # env steps the run had done when it was saved: warm-up, the anneal and the reports read t
if args.resume:
    first = int(load_run(args.resume, **run)["t"])
    print(f"resumed {args.resume} at step {first}")
t0 = time.perf_counter()
for t in range(first, args.steps):
    agent.select_action(mem.state, explore=explore, out=mem.action_slot())     # forward + exploration, into the ring's slot
    mem.step(polar=True, auto_reset="agent0_done", step_cap=1500, track_returns=True)
    if t + 1 == args.warmup or (args.resume and t == first and t + 1 > args.warmup):   # a resumed run captures again
        agent.capture(args.batch)                                              # sampling + the whole update, one graph
    if t + 1 >= args.warmup:
        if args.per_beta_final is not None:                                    # a device slot: the captured update follows it
            agent.set_per_beta(args.per_beta + (args.per_beta_final - args.per_beta) * t / max(1, args.steps - 1))
        agent.run(args.updates_per_step)
    if (t + 1) % args.report == 0 and agent.updates:
        rows, norms = agent.report(last=1)                                     # the one host read
        clip = "" if norms["critic"] is None else (f", critic grad norm {norms['critic'][0]:.4g} "
                                                   f"({norms['critic'][2] / agent.updates:.0%} of steps clipped)")
        q1, q2, pi = rows[0, :3]
        print(f"step {t + 1}: {agent.updates} updates, critic {q1:.4f} {q2:.4f} actor {pi:.4f}, "
              f"{(t + 1 - first) * args.envs / (time.perf_counter() - t0):,.0f} env steps/s{clip}")
    if args.save_every and (t + 1) % args.save_every == 0 and t + 1 < args.steps:
        save_run(args.save_run, **run, extra={"t": t + 1})
torch.cuda.synchronize()
if args.save_run:
    print("wrote", save_run(args.save_run, **run, extra={"t": max(first, args.steps)}))
st = venv.episode_stats()
print(f"{int(st['episodes'].sum())} episodes ended: {int(st['reach'].sum())} reached the goal, {int(st['coll'].sum())} collided")
if args.checkpoint:
    print("wrote", agent.save_checkpoint(args.checkpoint))
agent.close()
venv.close()

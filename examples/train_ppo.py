#!/usr/bin/env python3
"""A closed PPO training loop on the device ring: UAVVectorEnv builds the worlds, DeviceReplay(horizon=rollout) is the
rollout buffer the step launch writes into, PPO acts into the ring's action slot and updates from GAE(λ) advantages computed
over the ring in one HIP walk.  The host reads the losses and the episode statistics once per report.

    python examples/train_ppo.py [--envs 4096] [--agents 4] [--rollout 32] [--steps 3200] [--fused-heads]
                                [--normalize-obs] [--normalize-reward]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_uav_collision_avoidance_amd import UAVVectorEnv
from gym_uav_collision_avoidance_amd.checkpoint import load_run, save_run
from gym_uav_collision_avoidance_amd.ppo import PPO
from gym_uav_collision_avoidance_amd.replay import DeviceReplay

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--agents", type=int, default=4)
ap.add_argument("--rollout", type=int, default=32, help="env steps collected per update (the ring's horizon)")
ap.add_argument("--steps", type=int, default=3200, help="env steps in all; a multiple of --rollout")
ap.add_argument("--epochs", type=int, default=4)
ap.add_argument("--minibatches", type=int, default=4)
ap.add_argument("--lr", type=float, default=3e-4)
ap.add_argument("--gamma", type=float, default=0.99)
ap.add_argument("--lam", type=float, default=0.95)
ap.add_argument("--clip", type=float, default=0.2)
ap.add_argument("--ent-coef", type=float, default=0.0)
ap.add_argument("--max-grad-norm", type=float, default=0.5)
ap.add_argument("--report", type=int, default=10, help="updates between reports")
ap.add_argument("--fused-heads", action="store_true",
                help="sample and evaluate the losses in HIP between torch's GEMMs (libuavx_ppo.so, DESIGN.md §29)")
ap.add_argument("--normalize-obs", action="store_true",
                help="the networks see observations normalised by running statistics (libuavx_norm.so, DESIGN.md §30)")
ap.add_argument("--normalize-reward", action="store_true",
                help="GAE reads rewards divided by the running standard deviation of the discounted return (DESIGN.md §30)")
ap.add_argument("--save-run", type=str, default=None, metavar="FILE",
                help="write the whole run (worlds, ring, learner, generator, step) to FILE at the end (DESIGN.md §27)")
ap.add_argument("--resume", type=str, default=None, metavar="FILE",
                help="continue the run saved in FILE, built from the same arguments, up to --steps steps in all")
args = ap.parse_args()
if args.steps % args.rollout:
    ap.error("--steps must be a multiple of --rollout")

dev = torch.device("cuda", 0)
torch.manual_seed(0)           # the networks' initial weights: a run and the same run started again begin alike
venv = UAVVectorEnv(args.envs, num_agents=args.agents, device=dev, seed=0)
mem = DeviceReplay(venv.env, horizon=args.rollout)
mem.begin(venv.reset())
gen = torch.Generator(device=dev).manual_seed(0)
agent = PPO(mem, generator=gen, lr=args.lr, gamma=args.gamma, lam=args.lam, clip=args.clip, epochs=args.epochs,
            minibatches=args.minibatches, ent_coef=args.ent_coef, max_grad_norm=args.max_grad_norm,
            fused_heads=args.fused_heads, normalize_obs=args.normalize_obs, normalize_reward=args.normalize_reward)

run = dict(env=venv.env, memory=mem, agent=agent, generator=gen)
first = 0                      # env steps the run had done when it was saved
if args.resume:
    first = int(load_run(args.resume, **run)["t"])
    print(f"resumed {args.resume} at step {first}")
t0 = time.perf_counter()
for t in range(first, args.steps):
    agent.act()                                                                # the policy writes the ring's action slot
    mem.step(polar=True, auto_reset="agent0_done", step_cap=1500, track_returns=True)
    if (t + 1) % args.rollout == 0:
        losses = agent.update()
        if agent.updates % args.report == 0:
            row = {k: float(v) for k, v in losses.items()}                     # the one host read
            n, mean, std = (float(x) for x in agent.advantages.stats)
            print(f"step {t + 1}: {agent.updates} updates, policy {row['policy_loss']:.4f} value {row['value_loss']:.4f} "
                  f"entropy {row['entropy']:.4f}, {int(n)} advantages mean {mean:.4f} std {std:.4f}, "
                  f"{(t + 1 - first) * args.envs / (time.perf_counter() - t0):,.0f} env steps/s")
torch.cuda.synchronize()
if args.save_run:
    print("wrote", save_run(args.save_run, **run, extra={"t": max(first, args.steps)}))
st = venv.episode_stats()
print(f"{int(st['episodes'].sum())} episodes ended: {int(st['reach'].sum())} reached the goal, {int(st['coll'].sum())} collided")
agent.close()
venv.close()

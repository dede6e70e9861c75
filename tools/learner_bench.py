#!/usr/bin/env python3
"""Times one graph-captured learner update (sampling included) two ways in one process: FusedSAC / FusedTD3 / FusedDDPG
(learners.py: capture + run) and the same update hand-composed from the public classes of DESIGN §13-§18 as a user had to
write it before -- FusedReplaySampler, FusedTarget, FusedCriticLoss, FusedAdam (SAC's soft update inside the critic's step, as
FusedSAC runs it), FusedPolicyGrad, soft_update, and for SAC torch's Adam(capturable=True) on log_alpha with
alpha = log_alpha.exp(), no loss record.  The two take turns three times
(median, min, max of 30 replays each); TD3's replays alternate its critic-only and full graphs, so its figure is the mean
update.  One JSON line per (learner, rows), carrying the library's actor_sha.

    python tools/learner_bench.py [--rows 256 4096] [--iters 30] [--out profiles/r15_learner_bench.jsonl]
    rocprofv3 --kernel-trace --stats -d out -- python tools/learner_bench.py --rows 256 --only-new 50
        # the launches' own times: only the learners' graphs run, 50 updates each
    python tools/learner_bench.py --rows 256 --eager-host 300 --against PARENT_CHECKOUT [--turns 3] [--out FILE]
        # host wall time per ENQUEUED eager update_batch (explicit batch, synchronised only around the timed block): what
        # the Python bindings cost.  This tree and another checkout (built) take turns, one fresh process per turn; one
        # JSON line per learner with both side by side.  Without --against: this tree alone, one turn in this process.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_early = argparse.ArgumentParser(add_help=False)
_early.add_argument("--package-root", default=ROOT)
PACKAGE_ROOT = os.path.abspath(_early.parse_known_args()[0].package_root)
sys.path.insert(0, PACKAGE_ROOT)
import gym_uav_collision_avoidance_amd   # noqa: E402,F401 -- imported before the tools below put ROOT first
sys.path.insert(0, os.path.join(ROOT, "tools"))
from action_grad_bench import alternated                                          # noqa: E402
from critic_bench import PAIRS                                                    # noqa: E402
from critic_grad_bench import graphed                                             # noqa: E402
from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D, _actor_lib, learners      # noqa: E402
from gym_uav_collision_avoidance_amd.fused_critic import FusedCriticLoss, FusedTarget          # noqa: E402
from gym_uav_collision_avoidance_amd.fused_optim import FusedAdam, soft_update    # noqa: E402
from gym_uav_collision_avoidance_amd.fused_policy_grad import FusedPolicyGrad     # noqa: E402
from gym_uav_collision_avoidance_amd.fused_replay import FusedReplaySampler       # noqa: E402
from gym_uav_collision_avoidance_amd.replay import DeviceReplay                   # noqa: E402

CLASSES = {"sac": learners.FusedSAC, "td3": learners.FusedTD3, "ddpg": learners.FusedDDPG}


def memory(dev, envs=256, agents=4, horizon=64):
    env = BatchedMultiUAVWorld2D(envs, num_agents=agents, device=dev, seed=1)
    mem = DeviceReplay(env, horizon=horizon)
    mem.begin(env.reset())
    g = torch.Generator(device=dev).manual_seed(2)
    for _ in range(horizon + 8):
        mem.action_slot().copy_(torch.rand((envs, agents, 2), generator=g, device=dev) * 2 - 1)
        mem.step(polar=True, auto_reset="agent0_done", step_cap=40)
    return env, mem


class HandComposed:
    """The update as the parent's public classes compose it; replay() runs one update like a learner's run(1)."""

    def __init__(self, kind, mem, rows, dev):
        acls, ccls = PAIRS[kind]
        torch.manual_seed(0)
        self.kind, self.rows, self.updates = kind, rows, 0
        self.gen = None                      # the default generator: torch.cuda.graph registers it itself
        actor, critic, critic_t = acls().to(dev), ccls().to(dev), ccls().to(dev)
        critic_t.load_state_dict(critic.state_dict())
        ddpg = kind == "ddpg"
        self.sampler = FusedReplaySampler(mem).reserve(rows).push_count()
        self.bufs = tuple(torch.empty_like(t) for t in self.sampler.sample(rows, generator=self.gen))
        self.closs, self.pg = FusedCriticLoss(critic).reserve(rows), FusedPolicyGrad(actor, critic).reserve(rows)
        self.y = torch.empty((rows, 1), device=dev)
        self.critic, self.critic_t, self.tau = critic, critic_t, 5e-3
        if kind == "sac":
            self.target = FusedTarget(actor, critic_t)
            self.copt = FusedAdam(torch.optim.Adam(critic.parameters(), lr=3e-4), target=critic_t, tau=self.tau)
            self.aopt = FusedAdam(torch.optim.Adam(actor.parameters(), lr=3e-4))
            self.alpha = torch.full((1,), 2.0, device=dev)
            self.log_alpha = torch.zeros(1, requires_grad=True, device=dev)
            self.log_alpha.grad = torch.zeros(1, device=dev)
            self.alpha_optim = torch.optim.Adam([self.log_alpha], lr=3e-4, capturable=True)
        else:
            actor_t = acls().to(dev)
            actor_t.load_state_dict(actor.state_dict())
            self.target = FusedTarget(actor_t, critic_t)
            self.copt = FusedAdam(torch.optim.Adam(critic.parameters(), lr=1e-3 if ddpg else 3e-4, amsgrad=ddpg))
            self.aopt = FusedAdam(torch.optim.Adam(actor.parameters(), lr=1e-4 if ddpg else 3e-4, amsgrad=ddpg),
                                  target=actor_t, tau=self.tau)
        variants = (True, False) if kind == "td3" else (True,)
        self.graphs = {full: graphed(lambda full=full: self.update(full)) for full in variants}

    def update(self, full):
        s, a, r, s2, m = self.sampler.sample(self.rows, generator=self.gen, out=self.bufs, device_count=True)
        if self.kind == "sac":
            y = self.target(s2, r, m, alpha=self.alpha, generator=self.gen, out=self.y)
            self.closs.backward(s, a, y)
            self.copt.step(update_target=True)              # the soft update in the Adam launch, as FusedSAC does it
            self.pg.backward(s, alpha=self.alpha, generator=self.gen)
            self.aopt.step()
            with torch.no_grad():
                self.log_alpha.grad.copy_(-(self.pg.log_pi_mean + -2.0))      # d alpha_loss / d log_alpha, sac.py:82
                self.alpha_optim.step()
                self.alpha.copy_(self.log_alpha.exp())
            self.target.refresh()
            return
        y = self.target(s2, r, m, generator=self.gen, out=self.y)
        self.closs.backward(s, a, y)
        self.copt.step(update_target=False)
        if full:
            self.pg.backward(s)
            self.aopt.step(update_target=True)
            soft_update(self.critic_t, self.critic, self.tau)
            self.target.refresh()

    def replay(self):
        self.sampler.push_count()
        self.graphs[self.kind != "td3" or self.updates % 2 == 0].replay()
        self.updates += 1


class New:
    def __init__(self, kind, mem, rows, dev):
        torch.manual_seed(0)
        self.agent = CLASSES[kind](device=dev, memory=mem)
        self.agent.capture(rows)

    def replay(self):
        self.agent.run(1)


def eager_host(kind, rows, n, dev):
    """Host microseconds per enqueued update_batch of a learner on an explicit batch (and with the queue drained)."""
    torch.manual_seed(0)
    agent = CLASSES[kind](device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    g = torch.Generator(device=dev).manual_seed(2)
    batch = (torch.randn((rows, 10), generator=g, device=dev), torch.rand((rows, 2), generator=g, device=dev) * 2 - 1,
             torch.randn((rows,), generator=g, device=dev), torch.randn((rows, 10), generator=g, device=dev),
             torch.ones((rows, 1), device=dev))
    agent.reserve(rows)
    for _ in range(50):
        agent.update_batch(*batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        agent.update_batch(*batch)
    t1 = time.perf_counter()          # host time to ENQUEUE n updates
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    finite = bool(torch.isfinite(torch.from_numpy(agent.losses(last=1))).all())
    agent.close()
    return dict(host_us_per_update=(t1 - t0) / n * 1e6, us_per_update_incl_drain=(t2 - t0) / n * 1e6, finite=finite)


def eager_host_turn(a, dev):
    """One turn in this process: {learner: {rows: figures}} of the package this process imported."""
    return {kind: {str(rows): eager_host(kind, rows, a.eager_host, dev) for rows in a.rows} for kind in a.learners}


def eager_host_ab(a):
    """The other checkout and this tree alternating, a fresh process per turn; one JSON line per (learner, rows)."""
    arms = (("parent", os.path.abspath(a.against)), ("tree", ROOT))
    turns = {name: [] for name, _ in arms}
    for _ in range(a.turns):
        for name, root in arms:
            cmd = [sys.executable, os.path.abspath(__file__), "--package-root", root, "--eager-host", str(a.eager_host),
                   "--rows", *map(str, a.rows), "--learners", *a.learners]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
            turns[name].append(json.loads(out.strip().splitlines()[-1]))
    lines = []
    for kind in a.learners:
        for rows in a.rows:
            res = dict(learner=kind, rows=rows, updates_per_turn=a.eager_host, turns=a.turns)
            for name, _ in arms:
                ts = turns[name]
                us = [t["figures"][kind][str(rows)]["host_us_per_update"] for t in ts]
                res[name + "_actor_sha"], res[name + "_host_us_per_update"] = ts[0]["actor_sha"], us
                res[name + "_median_us"] = statistics.median(us)
                res[name + "_finite"] = all(t["figures"][kind][str(rows)]["finite"] for t in ts)
            res["tree_median_within_or_below_parent_range"] = res["tree_median_us"] <= max(res["parent_host_us_per_update"])
            lines.append(json.dumps(res))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=ROOT, help="import the package from this checkout instead of the tool's own")
    ap.add_argument("--eager-host", type=int, default=0, metavar="N",
                    help="time the host cost of N eager update_batch calls per learner instead of the graphs")
    ap.add_argument("--against", default=None, metavar="DIR",
                    help="with --eager-host: a built checkout of another commit that takes turns with this tree")
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--label", default=None, help="written into every graph-timing line as its `build` key")
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--learners", nargs="+", default=list(CLASSES))
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--only-new", type=int, default=0, metavar="N",
                    help="run only the learners' captured updates, N each (for a kernel trace)")
    a = ap.parse_args()
    if a.eager_host and a.against:          # the driver opens no GPU itself: one process at a time holds it
        for line in eager_host_ab(a):
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        return
    dev = torch.device("cuda", 0)
    sha = _actor_lib.source_hash()
    if a.eager_host:
        print(json.dumps(dict(package=PACKAGE_ROOT, actor_sha=sha, figures=eager_host_turn(a, dev))), flush=True)
        return
    env, mem = memory(dev)
    for rows in a.rows:
        for kind in a.learners:
            new = New(kind, mem, rows, dev)
            if a.only_new:
                new.agent.run(a.only_new)
                torch.cuda.synchronize()
                new.agent.close()
                continue
            base = HandComposed(kind, mem, rows, dev)
            res = dict(learner=kind, rows=rows, actor_sha=sha, iters=a.iters)
            if a.label:
                res = dict(build=a.label, **res)
            for k, v in alternated(dict(update_new_graph_us=new, update_hand_composed_graph_us=base), a.iters).items():
                res[k], res[k + "_min_max"] = v[0], v[1:]
            res["new_minus_hand_composed_us"] = res["update_new_graph_us"] - res["update_hand_composed_graph_us"]
            res["new_vs_hand_composed"] = res["update_new_graph_us"] / res["update_hand_composed_graph_us"]
            rec = new.agent.losses(last=1)
            res["finite"] = bool(torch.isfinite(torch.from_numpy(rec)).all())
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            new.agent.close()
            del new, base
            torch.cuda.empty_cache()
    env.close()


if __name__ == "__main__":
    main()

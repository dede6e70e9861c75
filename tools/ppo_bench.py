#!/usr/bin/env python3
"""Times PPO's HIP heads against the torch ops of ppo.py they replace, and one train_ppo.py iteration at
4 096 x 4 x 32 with fused_heads off and on.

  heads       sample at 16 384 rows against act()'s torch ops after the policy's forward; loss at 131 072 and 8 192 rows
              against a minibatch's gathers, losses and their backward down to (μ, log σ, V), on leaves that stand for the
              networks' outputs.  Three alternating rounds (min / median / max); the torch side is timed as two cases, whose
              spread is the noise.
  iteration   acting, stepping, advantages and the update of train_ppo.py's loop, median of five iterations per round, rings
              written by real env steps, rounds alternating torch, fused, torch, fused.  The torch path is the code as it
              was, so timing it is timing the baseline; the spread of its two rounds is the noise.
  gemm share  one fused update under torch.profiler: the share of device time in GEMM kernels (recorded as not measured if
              the profiler is not available).

Writes profiles/ppo_bench.json (one object) and prints it.

    python tools/ppo_bench.py [--out profiles/ppo_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gae_bench import rounds                                                        # noqa: E402
from gym_uav_collision_avoidance_amd import UAVVectorEnv, _ppo_lib                  # noqa: E402
from gym_uav_collision_avoidance_amd.ppo import PPO, log_prob                       # noqa: E402
from gym_uav_collision_avoidance_amd.ppo_heads import PPOHeads                      # noqa: E402
from gym_uav_collision_avoidance_amd.replay import DeviceReplay                     # noqa: E402

CLIP, VF, ENT = 0.2, 0.5, 0.0


def _verdict(res, hip, torch_a, torch_b):
    a, b = res[torch_a][1], res[torch_b][1]
    res["noise_us"] = round(abs(a - b), 2)
    res["speedup"] = round(min(a, b) / res[hip][1], 1)
    res["beats_torch_by_more_than_noise"] = bool(res[hip][1] + abs(a - b) < min(a, b))
    return res


def sample_head(rows, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    mean = torch.randn((rows, 2), generator=g, device=dev)
    log_std = torch.rand((rows, 2), generator=g, device=dev) * 5 - 4
    eps = torch.randn((rows, 2), generator=g, device=dev)
    u, logp, act = torch.zeros((rows, 2), device=dev), torch.zeros(rows, device=dev), torch.zeros((rows, 2), device=dev)
    u2, logp2, act2 = torch.zeros_like(u), torch.zeros_like(logp), torch.zeros_like(act)
    heads = PPOHeads(dev)

    def torch_ops():                                  # ppo.py act(), after the forward and the randn
        x = mean + log_std.exp() * eps
        u2.copy_(x)
        logp2.copy_(log_prob(mean, log_std, x))
        torch.tanh(x, out=act2)

    hip = lambda: heads.sample(mean, log_std, eps, u, logp, act)
    hip(), torch_ops()
    torch.cuda.synchronize()
    agrees = dict(u=float((u - u2).abs().max()), logp=float((logp - logp2).abs().max()), action=float((act - act2).abs().max()))
    res = rounds({"hip": hip, "torch_a": torch_ops, "torch_b": torch_ops}, {"hip": 500, "torch_a": 100, "torch_b": 100})
    res.update(rows=rows, max_abs_difference=agrees)
    return _verdict(res, "hip", "torch_a", "torch_b")


def loss_head(B, dev):
    g = torch.Generator(device=dev).manual_seed(2)
    R = 4 * B
    idx = torch.randperm(R, generator=g, device=dev)[:B]
    mean = torch.randn((B, 2), generator=g, device=dev)
    log_std = torch.rand((B, 2), generator=g, device=dev) * 2 - 1.5
    v = torch.randn(B, generator=g, device=dev)
    u = torch.randn((R, 2), generator=g, device=dev)
    u[idx] = mean + log_std.exp() * torch.randn((B, 2), generator=g, device=dev)
    logp_old = torch.zeros(R, device=dev)
    logp_old[idx] = log_prob(mean, log_std, u[idx]) + torch.rand(B, generator=g, device=dev) * 0.8 - 0.4
    adv, ret = torch.randn(R, generator=g, device=dev), torch.randn(R, generator=g, device=dev)
    weight = (torch.rand(R, generator=g, device=dev) > 0.1).float()
    heads = PPOHeads(dev)
    leaves = [t.clone().requires_grad_() for t in (mean, log_std, v)]

    def torch_ops():                                  # ppo.py update(), one minibatch between the forwards and the backward
        m, l, val = leaves
        for t in leaves:
            t.grad = None
        w = weight[idx]
        denom = w.sum().clamp(min=1.0)
        logp = log_prob(m, l, u[idx])
        ratio = torch.exp(logp - logp_old[idx])
        a = adv[idx]
        surrogate = torch.minimum(ratio * a, ratio.clamp(1.0 - CLIP, 1.0 + CLIP) * a)
        policy_loss = -(w * surrogate).sum() / denom
        value_loss = (w * (0.5 * (val - ret[idx]) ** 2)).sum() / denom
        entropy = -(w * logp).sum() / denom
        (policy_loss + VF * value_loss - ENT * entropy).backward()
        return policy_loss, value_loss, entropy

    hip = lambda: heads.loss(mean, log_std, v, idx, u, logp_old, adv, ret, weight, CLIP, VF, ENT)
    out, want = hip(), torch_ops()
    torch.cuda.synchronize()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    agrees = dict(policy_loss=rel(out.policy_loss, want[0].detach()), value_loss=rel(out.value_loss, want[1].detach()),
                  entropy=rel(out.entropy, want[2].detach()), g_mean=rel(out.g_mean, leaves[0].grad),
                  g_log_std=rel(out.g_log_std, leaves[1].grad), g_v=rel(out.g_v, leaves[2].grad))
    res = rounds({"hip": hip, "torch_a": torch_ops, "torch_b": torch_ops}, {"hip": 300, "torch_a": 30, "torch_b": 30})
    res.update(rows=B, gathered_from=R, max_relative_difference=agrees)
    return _verdict(res, "hip", "torch_a", "torch_b")


def _learner(dev, fused, envs, agents, rollout):
    torch.manual_seed(0)
    venv = UAVVectorEnv(envs, num_agents=agents, device=dev, seed=0)
    mem = DeviceReplay(venv.env, horizon=rollout)
    mem.begin(venv.reset())
    return venv, mem, PPO(mem, generator=torch.Generator(device=dev).manual_seed(0), fused_heads=fused)


def iteration(dev, fused, envs=4096, agents=4, rollout=32, iterations=5):
    """Median over `iterations` iterations of the phases of examples/train_ppo.py's loop, in µs."""
    venv, mem, ppo = _learner(dev, fused, envs, agents, rollout)
    phases = {k: [] for k in ("acting", "stepping", "update_total", "advantages")}
    first = None

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    for it in range(iterations + 1):
        marks = {k: [] for k in phases}
        for _ in range(rollout):
            marks["acting"].append(timed(ppo.act))
            marks["stepping"].append(timed(lambda: mem.step(polar=True, auto_reset="agent0_done", step_cap=1500)))
        losses = []
        marks["update_total"].append(timed(lambda: losses.append(ppo.update())))
        marks["advantages"].append(timed(lambda: ppo.advantages.compute(ppo.values)))
        torch.cuda.synchronize()
        if it:                                        # the first iteration warms everything up
            for k, v in marks.items():
                phases[k].append(sum(a.elapsed_time(b) for a, b in v) * 1e3)
        else:
            first = {k: float(v) for k, v in losses[0].items()}
    med = {k: round(sorted(v)[len(v) // 2], 1) for k, v in phases.items()}
    med["update"] = round(med["update_total"] - med["advantages"], 1)
    med["iteration"] = round(med["acting"] + med["stepping"] + med["update_total"], 1)
    med.update(fused_heads=fused, first_update_losses=first)
    venv.close()
    return med


def gemm_share(dev, envs=4096, agents=4, rollout=32):
    """The share of one fused update's device time that GEMM kernels hold, by torch.profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        venv, mem, ppo = _learner(dev, True, envs, agents, rollout)
        for it in range(2):
            for _ in range(rollout):
                ppo.act()
                mem.step(polar=True, auto_reset="agent0_done", step_cap=1500)
            if it == 0:
                ppo.update()
                torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            ppo.update()
            torch.cuda.synchronize()
        kernels = {}
        for ev in prof.events():
            on_device = getattr(ev, "device_type", None) is not None and "cuda" in str(ev.device_type).lower()
            if on_device and not getattr(ev, "is_user_annotation", False) and not ev.name.startswith(("Optimizer.", "ProfilerStep")):
                kernels[ev.name] = kernels.get(ev.name, 0.0) + float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0))
        venv.close()
        total = sum(kernels.values())
        if total <= 0:
            return dict(measured=False, why="the profiler recorded no device time")
        is_gemm = lambda n: "cijk" in n.lower() or "gemm" in n.lower()
        gemm = sum(t for n, t in kernels.items() if is_gemm(n))
        heads = sum(t for n, t in kernels.items() if "uavx_ppo_k" in n)
        top = sorted(kernels.items(), key=lambda kv: -kv[1])[:12]
        return dict(measured=True, device_time_us=round(total, 1), gemm_us=round(gemm, 1), gemm_share=round(gemm / total, 4),
                    heads_us=round(heads, 1), top_kernels=[[n[:90], round(t, 1)] for n, t in top])
    except Exception as e:                            # a measuring aid: its absence is recorded, not hidden
        return dict(measured=False, why=f"{type(e).__name__}: {e}"[:300])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_bench.json"))
    ap.add_argument("--no-profile", action="store_true", help="skip the torch.profiler pass")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(unit="us: heads [min, median, max] of 3 alternating rounds per call, eager, host launch cost included; "
                    "iteration phases are medians of 5 iterations per round",
               ppo_sha=_ppo_lib.source_hash(), device=torch.cuda.get_device_name(0),
               sample=[sample_head(16384, dev)], loss=[loss_head(131072, dev), loss_head(8192, dev)])
    its = [iteration(dev, fused) for fused in (False, True, False, True)]
    base = [r["iteration"] for r in its if not r["fused_heads"]]
    fused = [r["iteration"] for r in its if r["fused_heads"]]
    res["iteration_4096x4x32"] = dict(rounds=its, baseline_noise_us=round(abs(base[0] - base[1]), 1),
                                      baseline_us=round(min(base), 1), fused_us=round(sorted(fused)[0], 1),
                                      fused_rounds_us=fused, baseline_rounds_us=base,
                                      no_slower_than_baseline_plus_noise=bool(max(fused) <= min(base) + abs(base[0] - base[1])))

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    dump()                                            # the timings are kept whatever the profiler pass does
    if not a.no_profile:
        res["fused_update_gemm_share"] = gemm_share(dev)
        dump()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

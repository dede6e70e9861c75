"""What ppo.PPO computes, restated for the tests from its module docstring and DESIGN.md §28: plain torch on the CPU in a
dtype of the caller's (float64 is the reference; the same code in float32 measures what float32 arithmetic alone costs),
on deep copies of the two networks.  Nothing here calls into ppo.py: the log density, the 0/1 weight (a Python loop over the
ring's rows), the clipped surrogate, the value and entropy terms, the Σ w·x / max(1, Σ w) means, the gradients by autograd and
the global-norm clip are all written out again.  adv_norm and ret are gae_ref's."""
import copy
import math

import numpy as np
import torch

import gae_ref


def log_density_terms(mean, log_std, u):
    """The terms of log π(tanh(u)) per action dimension, [..., 2] each, signs included: the Gaussian's log density at u
    (three terms) minus log(1 − tanh²(u)) = log 4 − 2|u| − 2·log1p(exp(−2|u|)) (three terms, even in u)."""
    a = u.abs()
    z = (u - mean) / torch.exp(log_std)
    return [-0.5 * z * z, -log_std, torch.full_like(u, -0.5 * math.log(2.0 * math.pi)),
            torch.full_like(u, -math.log(4.0)), 2.0 * a, 2.0 * torch.log1p(torch.exp(-2.0 * a))]


def log_density(mean, log_std, u):
    """(log π summed over the action dimensions, Σ |terms|)."""
    terms = log_density_terms(mean, log_std, u)
    return sum(terms).sum(-1), sum(t.abs() for t in terms).sum(-1)


def networks(ppo, dtype):
    """Deep copies of the learner's policy and value net on the CPU in `dtype`."""
    return copy.deepcopy(ppo.policy).to("cpu", dtype), copy.deepcopy(ppo.value).to("cpu", dtype)


def weight_loop(done, skip, ended, count, steps, learners):
    """[steps, E, learners] float32, oldest step first.  A row is a sample unless it is a re-initialisation row or its agent was
    already done before the step: the row of step k − 1 has the agent's done bit, and that row neither ended the env's
    episode nor was a re-initialisation row itself.  Step 0 has no row before it.  skip / ended: [L, E] arrays, or both
    None for the flags in bits 1 and 2 of done[:, :, 0]."""
    L, E, _ = done.shape
    is_skip = lambda k, e: bool(done[k % L, e, 0] & 2) if skip is None else bool(skip[k % L, e])
    is_ended = lambda k, e: bool(done[k % L, e, 0] & 4) if ended is None else bool(ended[k % L, e])
    w = np.zeros((steps, E, learners), np.float32)
    why = np.zeros((steps, E, learners), np.uint8)      # 1 sample, 2 re-initialisation row, 3 parked, 4 kept by ended, 5 by skip
    for n, k in enumerate(range(count - steps, count)):
        for e in range(E):
            for i in range(learners):
                if is_skip(k, e):
                    why[n, e, i] = 2
                    continue
                was_done = k >= 1 and bool(done[(k - 1) % L, e, i] & 1)
                if was_done and not is_ended(k - 1, e) and not is_skip(k - 1, e):
                    why[n, e, i] = 3
                    continue
                w[n, e, i] = 1.0
                why[n, e, i] = 1 if not was_done else (4 if is_ended(k - 1, e) else 5)
    return w, why


def batch(mem, ppo, steps):
    """The inputs of an update as CPU tensors, rows in (step oldest first, env, learner) order: obs [R, 10], u [R, 2],
    logp_old [R], and the ring's arrays for gae_ref and weight_loop."""
    L, nl = mem.L, mem.num_learners
    slots = [k % L for k in range(mem.count - steps, mem.count)]
    cpu = lambda t: t.detach().cpu()
    ring = dict(rew=cpu(mem.rew).numpy(), done=cpu(mem.done).numpy(),
                skip=None if mem.packed else cpu(mem.skip).numpy(), ended=None if mem.packed else cpu(mem.ended).numpy())
    return dict(slots=slots, ring=ring, obs_ring=cpu(mem.obs), obs=cpu(mem.obs)[slots][:, :, :nl].reshape(-1, mem.obs.shape[-1]),
                u=cpu(ppo.u)[slots][:, :, :nl].reshape(-1, 2), logp_old=cpu(ppo.logp)[slots][:, :, :nl].reshape(-1),
                count=mem.count, steps=steps, learners=nl)


def update(b, policy, value, dtype, gamma=0.99, lam=0.95, clip=0.2, vf_coef=0.5, ent_coef=0.0, max_grad_norm=None, order=None):
    """One full-batch step's losses and gradients from batch() `b` on the given network copies.  order: a permutation of the
    rows to evaluate them in (PPO draws one per epoch; in exact arithmetic nothing depends on it), default as they lie.
    Returns a dict: weight [R] float32, ratio, adv [R] (all three in the ring's order), policy_loss, value_loss, entropy, loss
    (0-d), norm (the unclipped global gradient norm), grads (policy's then value's parameters, clipped)."""
    ring, steps, count, nl = b["ring"], b["steps"], b["count"], b["learners"]
    with torch.no_grad():
        values = value(b["obs_ring"].to(dtype)).squeeze(-1).to(torch.float32).numpy()
    adv, ret, valid = gae_ref.gae(values=values, count=count, steps=steps, gamma=gamma, lam=lam, learners=nl, **ring)
    norm, _ = gae_ref.normalise(adv, valid, count, steps)
    w, _ = weight_loop(ring["done"], ring["skip"], ring["ended"], count, steps, nl)
    take = lambda a: torch.from_numpy(a[b["slots"]][:, :, :nl].reshape(-1).copy())
    assert np.all(take(valid).numpy()[w.reshape(-1) > 0] == 1)                        # a sample is a valid row of the walk
    order = torch.arange(w.size) if order is None else order
    back = torch.argsort(order)
    w_t, a, r = torch.from_numpy(w.reshape(-1)).to(dtype)[order], take(norm).to(dtype)[order], take(ret).to(dtype)[order]
    obs, u, logp_old = b["obs"].to(dtype)[order], b["u"].to(dtype)[order], b["logp_old"].to(dtype)[order]
    denom = max(1.0, float(w.sum()))
    mean, log_std = policy(obs)
    logp, _ = log_density(mean, log_std, u)
    ratio = torch.exp(logp - logp_old)
    clipped = torch.where(ratio < 1.0 - clip, torch.full_like(ratio, 1.0 - clip),
                          torch.where(ratio > 1.0 + clip, torch.full_like(ratio, 1.0 + clip), ratio))
    objective = torch.where(ratio * a < clipped * a, ratio * a, clipped * a)          # the pessimistic of the two
    policy_loss = -(w_t * objective).sum() / denom
    v = value(obs).squeeze(-1)
    value_loss = (w_t * 0.5 * (v - r) * (v - r)).sum() / denom
    entropy = (w_t * -logp).sum() / denom
    loss = policy_loss + vf_coef * value_loss - ent_coef * entropy
    params = list(policy.parameters()) + list(value.parameters())
    grads = torch.autograd.grad(loss, params)
    total = torch.sqrt(sum((g.to(dtype) ** 2).sum() for g in grads))
    if max_grad_norm is not None:
        coef = min(1.0, float(max_grad_norm) / (float(total) + 1e-6))                 # torch's clip_grad_norm_
        grads = [g * coef for g in grads]
    return dict(weight=w.reshape(-1), policy_loss=policy_loss.detach(), value_loss=value_loss.detach(),
                entropy=entropy.detach(), loss=loss.detach(), ratio=ratio.detach()[back], adv=a[back], norm=float(total),
                grads=[g.detach() for g in grads])


def distance(x, ref):
    """max |x − ref| over the tensor, relative to max |ref|."""
    x, ref = torch.as_tensor(x).detach().cpu().to(torch.float64), torch.as_tensor(ref).detach().cpu().to(torch.float64)
    return float((x - ref).abs().max() / ref.abs().max().clamp(min=1e-300))

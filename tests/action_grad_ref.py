"""References for the tests of FusedActionGrad and FusedActorLoss: q and dq/da of every critic tower by torch.autograd.grad
in any dtype, the same written out layer by layer (include/uavx_action_grad.h's formulas, with an optional slope at exactly
z = 0), the learners' actor losses (model.py:88-99 and sac.py:70-75, td3.py:144, ddpg.py:77-78) in torch, and an autograd
function that stands where the fused one does but is built on the reference Jacobian."""
import copy

import torch

from grad_ref import towers
from gym_uav_collision_avoidance_amd import policy


def jacobian(module, s, a, dtype=torch.float64):
    """([q_t [B]], [dq_t/da [B, 2]]) per tower from torch itself: the module in `dtype`, autograd.grad with respect to a."""
    m = copy.deepcopy(module).to(dtype)
    s = s.detach().to(dtype)
    a = a.detach().to(dtype).requires_grad_(True)
    with torch.enable_grad():
        out = m(s, a)
        qs = list(out) if isinstance(out, tuple) else [out]
        js = [torch.autograd.grad(q.sum(), a, retain_graph=True)[0] for q in qs]   # rows are independent
    return [q.detach().squeeze(1) for q in qs], js


def analytic(module, s, a, dtype=torch.float64, kink_slope=None):
    """The same by the formulas of the header, in `dtype`.  kink_slope: the activation derivative used at exactly z = 0
    (None = torch's: relu 0, leaky 0.01)."""
    leaky = isinstance(module, policy.DDPGCritic)
    x = torch.cat([s, a], dim=-1).to(dtype)
    act = (lambda z: torch.where(z > 0, z, 0.01 * z)) if leaky else (lambda z: torch.where(z > 0, z, torch.zeros_like(z)))

    def dact(z):
        d = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.01 if leaky else 0.0))
        if kink_slope is not None:
            d = torch.where(z == 0, torch.full_like(z, kink_slope), d)
        return d

    qs, js = [], []
    for W1, b1, W2, b2, W3, b3 in towers(module):
        W1, b1, W2, b2, W3, b3 = (p.detach().to(dtype) for p in (W1, b1, W2, b2, W3, b3))
        z1 = x @ W1.T + b1
        z2 = act(z1) @ W2.T + b2
        qs.append((act(z2) @ W3.T + b3).squeeze(1))
        d2 = W3 * dact(z2)                                 # [B, h2]: the upstream gradient of q is 1
        d1 = (d2 @ W2) * dact(z1)
        js.append(d1 @ W1[:, 10:12])
    return qs, js


def actor(kind, seed, device="cpu", bias_scale=0.1):
    """A policy.py actor of the given learner with nonzero biases."""
    torch.manual_seed(seed)
    m = {"sac": policy.GaussianPolicy, "td3": policy.TD3Actor, "ddpg": policy.DDPGActor}[kind]()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.copy_(torch.randn_like(p) * bias_scale)
    return m.to(device)


def actor_preacts(kind, pol, s, dtype=torch.float64):
    """((z1, z2) of the actor's hidden layers, SAC's raw log-std before the clamp or None) in `dtype`."""
    m = copy.deepcopy(pol).to(dtype)
    s = s.to(dtype)
    l1, l2 = (m.linear1, m.linear2) if kind == "sac" else (m.l1, m.l2) if kind == "td3" else (m.input, m.fc1)
    act = torch.nn.functional.leaky_relu if kind == "ddpg" else torch.relu
    with torch.no_grad():
        z1 = l1(s)
        z2 = l2(act(z1))
        raw = m.log_std_linear(act(z2)) if kind == "sac" else None
    return (z1, z2), raw


def sac_sample(pol, s, noise):
    """policy.sample of model.py:88-99 with eps given: (action, log_pi [B, 1])."""
    mean, log_std = pol(s)
    std = log_std.exp()
    normal = torch.distributions.Normal(mean, std, validate_args=False)
    x_t = mean + std * noise
    y_t = torch.tanh(x_t)
    log_prob = normal.log_prob(x_t)
    log_prob = log_prob - torch.log(1.0 * (1 - y_t.pow(2)) + 1e-6)
    return y_t, log_prob.sum(1, keepdim=True)


def actor_loss(kind, pol, critic_fn, s, alpha=None, noise=None):
    """The trainer's actor loss with `critic_fn(s, a)` in the critic's place (the module itself, or a stand-in that
    returns what its forward returns): (loss, log_pi or None)."""
    if kind == "sac":
        a, log_pi = sac_sample(pol, s, noise)
        q1, q2 = critic_fn(s, a)
        return ((alpha * log_pi) - torch.min(q1, q2)).mean(), log_pi
    if kind == "td3":
        return -critic_fn(s, pol(s))[0].mean(), None         # critic.Q1
    return -critic_fn(s, pol(s)).mean(), None


def actor_grads(kind, pol, crit, s, alpha=None, noise=None, dtype=torch.float64, critic_fn=None):
    """([d loss / d p for the actor's parameters], loss, log_pi) by full torch autograd in `dtype` (critic_fn: a stand-in
    for the critic module, given the dtype copies of (critic, state) at call time)."""
    p2, c2 = copy.deepcopy(pol).to(dtype), copy.deepcopy(crit).to(dtype)
    for p in c2.parameters():
        p.requires_grad_(True)
    s = s.detach().to(dtype)
    noise = None if noise is None else noise.detach().to(dtype)
    fn = c2 if critic_fn is None else (lambda ss, aa: critic_fn(c2, ss, aa))
    loss, log_pi = actor_loss(kind, p2, fn, s, alpha, noise)
    gs = torch.autograd.grad(loss, list(p2.parameters()))
    return [g.detach() for g in gs], loss.detach(), None if log_pi is None else log_pi.detach()


class _SeamFn(torch.autograd.Function):
    """q of every tower as a function of the action alone: forward keeps the reference Jacobian, backward is
    sum_t g_t * J_t.  What FusedActionGrad's autograd function does, with `jacobian` where the kernel is."""

    @staticmethod
    def forward(ctx, a, module, s):
        qs, js = jacobian(module, s, a, a.dtype)
        ctx.js = js
        return tuple(q.unsqueeze(1) for q in qs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gs):
        return sum(g * j for g, j in zip(gs, ctx.js)), None, None


def seam_critic(module, s, a):
    """Stand-in for module(s, a) through _SeamFn: what the module's forward returns."""
    qs = _SeamFn.apply(a, module, s)
    return qs if len(qs) == 2 else qs[0]

"""PPO's sampling and loss heads (include/uavx_ppo.h) restated for the tests in plain torch on the CPU, in a
dtype of the caller's: float64 is the reference, the same code in float32 measures what float32 arithmetic alone costs.
Nothing here calls ppo.py or the library, and nothing uses autograd: the gradients are written out as the header writes
them.  make_case() draws the inputs the GPU tests run on."""
import math

import torch

_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
_LOG_2 = math.log(2.0)


def log_density(mean, log_std, u):
    """(log π summed over the action dimensions, z) in the header's form: the Gaussian's log density at u minus
    2·(log 2 − u − softplus(−2u)), softplus(x) = max(x, 0) + log1p(exp(−|x|))."""
    z = (u - mean) * torch.exp(-log_std)
    gauss = -0.5 * z * z - log_std - _HALF_LOG_2PI
    x = -2.0 * u
    softplus = torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-x.abs()))
    squash = 2.0 * ((_LOG_2 - u) - softplus)
    return (gauss - squash).sum(-1), z


def sample(mean, log_std, eps, dtype):
    """(u, tanh(u), log π(u)) of u = μ + σ·ε."""
    mean, log_std, eps = (t.detach().cpu().to(dtype) for t in (mean, log_std, eps))
    u = mean + torch.exp(log_std) * eps
    return u, torch.tanh(u), log_density(mean, log_std, u)[0]


def loss(mean, log_std, v, idx, u, logp_old, adv, ret, weight, clip, vf_coef, ent_coef, dtype, order=None):
    """The loss head on CPU copies of the inputs in `dtype`.  order: a permutation of the minibatch's rows to sum them in
    (per-row results are returned in the caller's order; in exact arithmetic nothing depends on it).  Returns a dict:
    ratio, g_mean, g_log_std, g_v, passes (bool), s1, s2, w per row; policy_loss, value_loss, entropy, n 0-d."""
    to = lambda t: t.detach().cpu().to(dtype)
    mean, log_std, v, u, logp_old, adv, ret, weight = map(to, (mean, log_std, v, u, logp_old, adv, ret, weight))
    B = v.shape[0]
    idx = torch.arange(B) if idx is None else idx.detach().cpu()
    order = torch.arange(B) if order is None else order
    back = torch.argsort(order)
    mean, log_std, v, idx = mean[order], log_std[order], v[order], idx[order]
    a, w, dv = adv[idx], weight[idx], v - ret[idx]
    logp, z = log_density(mean, log_std, u[idx])
    r = torch.exp(logp - logp_old[idx])
    lo, hi = 1.0 - clip, 1.0 + clip
    s1, s2 = r * a, torch.clamp(r, lo, hi) * a
    surr = torch.where(s1 < s2, s1, s2)
    n = w.sum()
    D = torch.clamp(n, min=1.0)
    policy_loss, value_loss, entropy = -(w * surr).sum() / D, (w * (0.5 * dv * dv)).sum() / D, -(w * logp).sum() / D
    passes = ((r >= lo) & (r <= hi)) | (s1 < s2)
    k = w / D
    g_lp = k * (ent_coef - torch.where(passes, a * r, torch.zeros_like(r)))
    g_mean = g_lp[:, None] * z * torch.exp(-log_std)
    g_log_std = g_lp[:, None] * (z * z - 1.0)
    g_v = k * vf_coef * dv
    rows = dict(ratio=r, g_mean=g_mean, g_log_std=g_log_std, g_v=g_v, passes=passes, s1=s1, s2=s2, w=w, adv=a, logp=logp)
    out = {name: t[back] for name, t in rows.items()}
    out.update(policy_loss=policy_loss, value_loss=value_loss, entropy=entropy, n=n)
    return out


ROW_QUANTITIES = ("ratio", "g_mean", "g_log_std", "g_v")
SCALARS = ("policy_loss", "value_loss", "entropy")


def make_case(B, seed, clip=0.2, identity=False):
    """The float32 inputs of one loss call, as CPU tensors: a minibatch of B rows drawn without repetition from R = 2B + 3.
    μ ~ N(0, 1); ℓ ~ U[−4, 1] with a few rows at exactly −20 and 2; u = μ + σ·N(0, 1) with a handful of |u| up to 20 (at
    rows of ℓ = 1, so that the sample stays one the policy could have drawn); adv ~ N(0, 1) with a few exact zeros; w 0/1,
    about a quarter zeros, the minibatch's last row always a sample with adv = 0.75 (so the last workgroup's partial is not
    zero); log π_old = the float64 density + U(±0.6), moved by 0.01 wherever the float64 ratio would come within 2e-3 of
    1 ± clip.  The flat arrays' other rows hold values of the same kind, so a wrong gather shows."""
    g = torch.Generator().manual_seed(seed)
    R = 2 * B + 3
    idx = torch.arange(B) if identity else torch.randperm(R, generator=g)[:B]
    mean = torch.randn((B, 2), generator=g)
    log_std = torch.rand((B, 2), generator=g) * 5.0 - 4.0
    v = torch.randn(B, generator=g)
    noise = torch.randn((B, 2), generator=g)
    few = max(1, B // 50)
    pick = lambda: torch.randperm(B, generator=g)[:few]
    log_std[pick(), 0] = -20.0
    log_std[pick(), 1] = 2.0
    far = pick()
    log_std[far] = 1.0
    u_rows = (mean.double() + torch.exp(log_std.double()) * noise.double()).float()
    u_rows[far, 0] = torch.linspace(-20.0, 20.0, far.numel()) if far.numel() > 1 else torch.tensor([20.0])
    u = torch.randn((R, 2), generator=g)
    u[idx] = u_rows
    adv = torch.randn(R, generator=g)
    adv[torch.randperm(R, generator=g)[:max(2, R // 40)]] = 0.0
    ret = torch.randn(R, generator=g)
    weight = (torch.rand(R, generator=g) >= 0.25).float()
    weight[idx[-1]] = 1.0                              # the last row is a sample: the last workgroup's partial counts
    adv[idx[-1]] = 0.75
    logp, _ = log_density(mean.double(), log_std.double(), u_rows.double())
    offset = torch.rand(B, generator=g, dtype=torch.float64) * 1.2 - 0.6
    for _ in range(3):
        old = (logp + offset).float()
        ratio = torch.exp(logp - old.double())
        near = ((ratio - (1.0 - clip)).abs() < 2e-3) | ((ratio - (1.0 + clip)).abs() < 2e-3)
        offset = torch.where(near, offset + 0.01, offset)
    logp_old = torch.randn(R, generator=g)
    logp_old[idx] = old
    return dict(mean=mean, log_std=log_std, v=v, idx=None if identity else idx, u=u, logp_old=logp_old, adv=adv, ret=ret,
                weight=weight)

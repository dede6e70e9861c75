"""Float64 statement of the Adam step and of the soft target update, for the tests of FusedAdam / soft_update
(include/uavx_optim.h).  Written from the formulas of Kingma & Ba's Algorithm 1 in the arrangement torch.optim.Adam uses
(bias corrections folded into the step size and the denominator), independent of the kernels; checked against
torch.optim.Adam on float64 CPU parameters in tests/test_optim_host.py."""
import math

import torch

SAC_SHAPES = [(256, 12), (256,), (256, 256), (256,), (1, 256), (1,)] * 2        # TwinQ / TD3TwinQ
DDPG_SHAPES = [(400, 12), (400,), (300, 400), (300,), (1, 300), (1,)]          # DDPGCritic


def adam_step(p, g, m, v, vmax, t, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """One step, t = the count AFTER this step (1 for the first).  p, g, m, v (and vmax, or None without AMSGrad): float64
    tensors, not modified.  Returns (p, m, v, vmax)."""
    assert all(x.dtype == torch.float64 for x in (p, g, m, v))
    m = m + (g - m) * (1.0 - beta1)
    v = v * beta2 + (g * g) * (1.0 - beta2)
    d = v
    if vmax is not None:
        vmax = torch.maximum(vmax, v)
        d = vmax
    step_size = lr / (1.0 - beta1 ** t)
    denom = d.sqrt() / math.sqrt(1.0 - beta2 ** t) + eps
    return p - step_size * (m / denom), m, v, vmax


def soft(target, source, tau):
    """target·(1 − tau) + source·tau in float64."""
    assert target.dtype == source.dtype == torch.float64
    return target * (1.0 - tau) + source * tau


def run(p0, grads, amsgrad, lr=3e-4, t0=0, state=None):
    """len(grads) steps over lists of float64 tensors from count t0.  state: optional (m, v, vmax) lists.  Returns
    (p, m, v, vmax) lists."""
    p = [x.clone() for x in p0]
    m, v, vmax = state if state is not None else ([torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p],
                                                  [torch.zeros_like(x) for x in p] if amsgrad else [None] * len(p))
    for k, gs in enumerate(grads):
        for i in range(len(p)):
            p[i], m[i], v[i], vmax[i] = adam_step(p[i], gs[i], m[i], v[i], vmax[i], t0 + k + 1, lr=lr)
    return p, m, v, vmax

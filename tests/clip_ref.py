"""Float64 statement of the clip of the global gradient norm and of the Adam step behind it (include/uavx_clip.h), for the
tests of FusedAdam(max_grad_norm=...).  Written from torch.nn.utils.clip_grad_norm_'s documentation -- one 2-norm over all
gradients, every gradient multiplied by clamp(max_norm / (norm + 1e-6), max=1) -- independent of the kernels; checked
against clip_grad_norm_ + torch.optim.Adam on float64 CPU parameters in tests/test_clip_host.py."""
import numpy as np
import torch

import optim_ref

EPS = 1e-6


def norm64(grads):
    """sqrt(sum of g.double()^2) over all tensors, as a Python float."""
    return float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))


def coef32(norm, max_norm):
    """The float32 coefficient from a float32 norm, in numpy float32 scalars: min(1, max_norm / (norm + 1e-6)), a NaN
    passing through.  Returns np.float32."""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm) + np.float32(EPS))
    return np.float32(1.0) if c > np.float32(1.0) else c


def coef64(norm, max_norm):
    """The same in float64 (a Python float), for the float64 comparison against torch."""
    c = max_norm / (norm + EPS)
    return 1.0 if c > 1.0 else c


def clipped_step(p, g, m, v, vmax, t, max_norm, **kw):
    """One clipped step over lists of float64 tensors (vmax: a list, or None without AMSGrad), t = the count AFTER this step.
    Returns (p, m, v, vmax lists, norm, coef)."""
    norm = norm64(g)
    c = coef64(norm, max_norm)
    out = [optim_ref.adam_step(p[i], g[i] * c, m[i], v[i], None if vmax is None else vmax[i], t, **kw) for i in range(len(p))]
    ps, ms, vs, xs = (list(col) for col in zip(*out))
    return ps, ms, vs, (None if vmax is None else xs), norm, c

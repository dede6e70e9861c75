"""Reference gradients of the WEIGHTED critic loss for the tests of FusedCriticLoss.backward(weight=,
q_out=): torch autograd, in any dtype, of  L_t = mean_b w_b (q_t − y)²  or  mean_b w_b |q_t − y|  on the policy.py critics
of grad_ref.py.  With every weight 1 it is grad_ref.autograd's loss (checked in tests/test_wgrad_host.py)."""
import copy

import torch

from grad_ref import critic, default_loss, params, towers  # noqa: F401  (the tests take critic, towers, params from here)


def autograd(module, s, a, y, w, loss=None, dtype=torch.float64):
    """(grads in params() order, [loss per tower], [q per tower, each [B]]) from torch itself: the module in `dtype`, the
    weighted loss, backward().  w: [B] or [B, 1]."""
    loss = loss or default_loss(module)
    m = copy.deepcopy(module).to(dtype)
    s, a, y, w = s.to(dtype), a.to(dtype), y.reshape(-1, 1).to(dtype), w.reshape(-1, 1).to(dtype)
    out = m(s, a)
    qs = list(out) if isinstance(out, tuple) else [out]
    if loss == "mse":
        ls = [(w * (q - y) ** 2).mean() for q in qs]
    else:
        ls = [(w * (y - q).abs()).mean() for q in qs]
    m.zero_grad()
    sum(ls).backward()
    return ([p.grad.detach().clone() for p in params(m)], [l.detach() for l in ls],
            [q.detach().reshape(-1).clone() for q in qs])

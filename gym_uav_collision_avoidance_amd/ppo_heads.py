"""PPO's sampling and loss heads in HIP (include/uavx_ppo.h, libuavx_ppo.so): what ppo.PPO does between its
networks' GEMMs.

    heads = PPOHeads(device)
    heads.sample(mean, log_std, eps, u_out, logp_out, action_out)            # one launch
    out = heads.loss(mean, log_std, v, idx, u, logp_old, adv, ret, weight, clip, vf_coef, ent_coef)     # two launches
    torch.autograd.backward([mean, log_std, v], [out.g_mean, out.g_log_std, out.g_v])

sample() turns the policy's (μ, log σ) and a noise draw into the pre-squash sample, its tanh and its log density; loss() turns
a minibatch's (μ, log σ, V) into the three weighted means of the clipped surrogate and the gradient of their sum with respect
to those outputs, which the caller hands to autograd.  The sums are float64 in an order the launch geometry fixes, so two
calls give the same bytes.  What loss() returns are views of persistent buffers, valid until the next call.  There is NO
fallback: a missing library or device raises."""
import collections
import ctypes
import math

import torch

Loss = collections.namedtuple("Loss", "policy_loss value_loss entropy n ratio g_mean g_log_std g_v")


def _rows(name, rows):
    if isinstance(rows, bool) or not isinstance(rows, int) or not 1 <= rows <= 2 ** 31 - 1:
        raise ValueError(f"uavx: PPOHeads: {name} must be an int in [1, 2^31 - 1], got {rows!r}")
    return rows


class PPOHeads:
    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = self._mod = None
        self._cap = 0
        self._ratio = self._g_mean = self._g_log_std = self._g_v = self._scalars = self._work = None

    # -- host-side checks: all of them come before the library is loaded -------------------------------------------------------
    def _tensor(self, name, t, shape, dtype=torch.float32):
        if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
            got = f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"uavx: PPOHeads: {name} must be {dtype} {tuple(shape)}, got {got}")
        if t.device != self.device or not t.is_contiguous():
            raise ValueError(f"uavx: PPOHeads: {name} must be contiguous and on {self.device}")
        return t

    @staticmethod
    def _coefficient(name, x, positive=False):
        ok = not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x) and (x > 0 if positive else x >= 0)
        if not ok:
            raise ValueError(f"uavx: PPOHeads: {name} must be a finite float {'> 0' if positive else '>= 0'}, got {x!r}")
        return float(x)

    def _bind(self):
        if self.device.type != "cuda":
            raise ValueError("uavx: PPOHeads launches on a GPU: there is no CPU path")
        if self._lib is None:
            from . import _ppo_lib
            self._mod, self._lib = _ppo_lib, _ppo_lib.load()

    def reserve(self, rows):
        """Sizes the persistent output buffers and the workspace for minibatches of up to `rows` rows (loss() grows them
        when it has to; what an earlier loss() returned is then no longer what the next one writes)."""
        rows = _rows("rows", rows)
        if rows <= self._cap:
            return
        self._bind()
        need = ctypes.c_int64(0)
        self._mod.check(self._lib.uavx_ppo_loss_workspace_bytes(rows, ctypes.byref(need)), "uavx_ppo_loss_workspace_bytes")
        dev = self.device
        self._ratio = torch.zeros(rows, dtype=torch.float32, device=dev)
        self._g_mean = torch.zeros((rows, 2), dtype=torch.float32, device=dev)
        self._g_log_std = torch.zeros((rows, 2), dtype=torch.float32, device=dev)
        self._g_v = torch.zeros(rows, dtype=torch.float32, device=dev)
        self._scalars = torch.zeros(4, dtype=torch.float32, device=dev)
        self._work = torch.zeros(need.value // 8, dtype=torch.float64, device=dev)
        self._cap = rows

    # -- the two heads ---------------------------------------------------------------------------------------------------------
    def sample(self, mean, log_std, eps, u_out, logp_out, action_out):
        """mean, log_std, eps [..., 2] -> u_out, action_out [..., 2], logp_out [...]: u = μ + σ·ε, tanh(u) and log π of the
        stored u.  All contiguous float32 on the device; the leading shape is the caller's.  One launch on the current
        stream."""
        if not torch.is_tensor(mean) or mean.dim() < 1 or mean.shape[-1] != 2 or mean.numel() == 0:
            got = tuple(mean.shape) if torch.is_tensor(mean) else type(mean).__name__
            raise ValueError(f"uavx: PPOHeads: mean must be float32 [..., 2], got {got}")
        shape = tuple(mean.shape)
        for name, t in (("mean", mean), ("log_std", log_std), ("eps", eps), ("u_out", u_out), ("action_out", action_out)):
            self._tensor(name, t, shape)
        self._tensor("logp_out", logp_out, shape[:-1])
        rows = _rows("rows", mean.numel() // 2)
        self._bind()
        with torch.cuda.device(self.device):
            rc = self._lib.uavx_ppo_sample(mean.data_ptr(), log_std.data_ptr(), eps.data_ptr(), rows, u_out.data_ptr(),
                                           logp_out.data_ptr(), action_out.data_ptr(),
                                           torch.cuda.current_stream(self.device).cuda_stream)
        self._mod.check(rc, "uavx_ppo_sample")

    def loss(self, mean, log_std, v, idx, u, logp_old, adv, ret, weight, clip, vf_coef, ent_coef):
        """mean, log_std [B, 2], v [B]: the minibatch's network outputs (detached).  idx [B] int64 or None: the rows of u
        [R, 2], logp_old, adv, ret, weight [R] the minibatch is made of (None: the first B).  Returns Loss(policy_loss,
        value_loss, entropy, n, ratio, g_mean, g_log_std, g_v): 0-d means, n = Σ weight, the probability ratio [B] and the
        gradient of policy_loss + vf_coef·value_loss − ent_coef·entropy with respect to mean, log_std and v.  Views of
        persistent buffers, valid until the next call.  Two launches on the current stream; nothing is read on the host."""
        if not torch.is_tensor(v) or v.dim() != 1 or v.numel() == 0:
            got = tuple(v.shape) if torch.is_tensor(v) else type(v).__name__
            raise ValueError(f"uavx: PPOHeads: v must be float32 [B], got {got}")
        if not torch.is_tensor(weight) or weight.dim() != 1 or weight.numel() == 0:
            got = tuple(weight.shape) if torch.is_tensor(weight) else type(weight).__name__
            raise ValueError(f"uavx: PPOHeads: weight must be float32 [R], got {got}")
        B, R = _rows("B", v.shape[0]), _rows("R", weight.shape[0])
        self._tensor("mean", mean, (B, 2)), self._tensor("log_std", log_std, (B, 2)), self._tensor("v", v, (B,))
        if idx is not None:
            self._tensor("idx", idx, (B,), torch.int64)
        elif B > R:
            raise ValueError(f"uavx: PPOHeads: without idx the minibatch's {B} rows must be the first of the {R} given")
        self._tensor("u", u, (R, 2))
        for name, t in (("logp_old", logp_old), ("adv", adv), ("ret", ret), ("weight", weight)):
            self._tensor(name, t, (R,))
        clip = self._coefficient("clip", clip, positive=True)
        vf_coef, ent_coef = self._coefficient("vf_coef", vf_coef), self._coefficient("ent_coef", ent_coef)
        self.reserve(B)
        out = Loss(self._scalars[0], self._scalars[1], self._scalars[2], self._scalars[3], self._ratio[:B], self._g_mean[:B],
                   self._g_log_std[:B], self._g_v[:B])
        with torch.cuda.device(self.device):
            rc = self._lib.uavx_ppo_loss(mean.data_ptr(), log_std.data_ptr(), v.data_ptr(),
                                         None if idx is None else idx.data_ptr(), B, u.data_ptr(), logp_old.data_ptr(),
                                         adv.data_ptr(), ret.data_ptr(), weight.data_ptr(), R, clip, vf_coef, ent_coef,
                                         self._ratio.data_ptr(), self._scalars.data_ptr(), self._g_mean.data_ptr(),
                                         self._g_log_std.data_ptr(), self._g_v.data_ptr(), self._work.data_ptr(),
                                         self._work.numel() * 8, torch.cuda.current_stream(self.device).cuda_stream)
        self._mod.check(rc, "uavx_ppo_loss")
        return out

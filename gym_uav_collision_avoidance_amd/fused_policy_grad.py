"""FusedPolicyGrad: the learners' actor-loss block, `zero_grad(); loss.backward()` of
    SAC   (alpha * log_pi - min(Q1, Q2)(s, pi(s))).mean()      (model.py:88-99, sac.py:70-78)
    TD3   -Q1(s, actor(s)).mean()                              (td3.py:144)
    DDPG  -Q(s, actor(s)).mean()                               (ddpg.py:77-79)
with the actor's own forward and backward in HIP as well (libuavx_actor.so, include/uavx_policy_grad.h): five launches, the
critic towers being the one launch of FusedActionGrad between the actor's forward and its backward.  FusedActorLoss
(fused_critic.py) computes the same block with the actor under torch autograd.

    pg = FusedPolicyGrad(actor, critic)        # the learner is told from the pair, as FusedActorLoss does
    loss, log_pi = pg.backward(s, alpha=alpha, generator=g)      # SAC; TD3 / DDPG: loss = pg.backward(s)
    actor_optim.step()
    a, log_pi = pg.act(s, noise=eps)           # launch 1 alone; keeps the activations in the workspace
    pg.backward_from(s, q, dqda, alpha=alpha)  # launches 3 to 5 alone, from q [T, B] and dq/da [T, B, 2]
    pg.reserve(rows)                           # workspace and output buffers before a graph capture
    pg.log_pi_mean                             # SAC: mean log_pi of the last backward, a 0-d device tensor

The calls read the actor's and the critic's LIVE float32 parameters when the kernels run: an optimiser step is seen by the
next call with no refresh.  Inputs must be float32 on the modules' device; anything else raises (no conversion, no CPU
path).  Every returned tensor is a VIEW of a persistent buffer, valid until the next call on the same object."""
import ctypes

import torch

from . import _actor_lib
from ._fused_common import (KIND_NAMES, ParamSlots, Workspace, actor_layers, alpha_arg, capture_guard, check_buffers,
                            check_on_gpu, critic_layers, noise_arg, rows2, stream)
from .fused_critic import FusedActionGrad, FusedCritic


class FusedPolicyGrad:
    """actor: the live GaussianPolicy / TD3Actor / DDPGActor.  critic: a TwinQ / TD3TwinQ / DDPGCritic, an f32 FusedCritic
    or a FusedActionGrad.  Only the actor's parameters get a .grad: one that is usable (float32, contiguous, the
    parameter's shape and device) is overwritten in place, otherwise a persistent buffer is assigned; the critic's
    parameters' .grad is not touched."""

    def __init__(self, actor, critic):
        found = actor_layers(actor)
        if found is None:
            raise TypeError(f"uavx: FusedPolicyGrad takes a GaussianPolicy, TD3Actor or DDPGActor, not {type(actor).__name__}")
        # the pair and the devices are checked on the host, before anything touches a device
        cmod = critic.module if isinstance(critic, (FusedActionGrad, FusedCritic)) else critic
        cfound = critic_layers(cmod)
        if cfound is None:
            raise TypeError(f"uavx: FusedPolicyGrad takes a TwinQ, TD3TwinQ, DDPGCritic, FusedCritic or FusedActionGrad as "
                            f"its critic, not {type(critic).__name__}")
        (kind, layers), ckind = found, cfound[0]
        if ckind != kind:
            raise TypeError(f"uavx: FusedPolicyGrad pairs a {KIND_NAMES[kind]} actor ({type(actor).__name__}) with a "
                            f"{KIND_NAMES[ckind]} critic ({type(cmod).__name__})")
        check_on_gpu(layers[0].weight.device, "FusedPolicyGrad", "actor")
        self._owned = None
        if not isinstance(critic, FusedActionGrad):
            critic = self._owned = FusedActionGrad(critic)
        params = [p for lin in layers for p in (lin.weight, lin.bias)]
        for p in params:
            if p is None or p.device != critic.device or p.dtype != torch.float32:
                self.close()
                raise ValueError(f"uavx: FusedPolicyGrad needs the actor in float32 on the critic's device {critic.device}, "
                                 f"a parameter is {getattr(p, 'dtype', None)} on {getattr(p, 'device', None)}")
        self.actor, self.critic, self.kind, self.device = actor, critic, kind, critic.device
        self.obs_dim, self.hidden1, self.hidden2 = layers[0].in_features, layers[0].out_features, layers[1].out_features
        self._lib = critic._lib
        self._slots = ParamSlots(params, 8, "FusedPolicyGrad", "actor")
        self._towers = critic.critic.towers
        self._mask = 3 if kind == _actor_lib.SAC else 1
        dev = self.device
        self._scalars = torch.zeros(2, dtype=torch.float32, device=dev)      # loss, mean log_pi
        self._ws = Workspace(dev)
        self._cap = 0                                                        # rows the output buffers hold
        self._action = self._logpi = self._q = self._j = None
        self._acted = 0                                                      # rows of the forward the workspace holds
        self._keep = None
        # the sizes are checked now (a hidden size no kernel is compiled for raises here, not at the first call)
        self.workspace_bytes(1)

    @property
    def learner(self):
        return KIND_NAMES[self.kind].lower()

    @property
    def log_pi_mean(self):
        """SAC: mean_b log_pi of the last backward / backward_from, a 0-d view of a persistent device buffer.  The gradient of
        alpha_loss (sac.py:82) with respect to log_alpha is -(log_pi_mean + target_entropy)."""
        if self.kind != _actor_lib.SAC:
            raise AttributeError("uavx: log_pi_mean exists for a SAC actor only")
        return self._scalars[1]

    def workspace_bytes(self, rows):
        n = ctypes.c_int64()
        rc = self._lib.uavx_policy_grad_workspace_bytes(self.kind, self.hidden1, self.hidden2, int(rows), ctypes.byref(n))
        _actor_lib.check(rc, f"uavx_policy_grad_workspace_bytes({KIND_NAMES[self.kind]}, {self.hidden1}, {self.hidden2}, "
                             f"{rows})")
        return n.value

    def reserve(self, rows):
        """Grows the workspace and the output buffers to what `rows` rows need (a graph capture cannot allocate them)."""
        rows = int(rows)
        if self._ws.reserve(self.workspace_bytes(rows)):
            self._acted = 0
        if self._cap < rows:
            dev, T = self.device, self._towers
            self._action = torch.zeros(rows * 2, dtype=torch.float32, device=dev)
            self._logpi = torch.zeros(rows, dtype=torch.float32, device=dev)
            self._q = torch.zeros(T * rows, dtype=torch.float32, device=dev)
            self._j = torch.zeros(T * rows * 2, dtype=torch.float32, device=dev)
            self._cap = rows
        return self

    def _ready(self, rows):
        if self._cap < rows or self._ws.buf.numel() < self.workspace_bytes(rows):
            capture_guard("workspace", rows)
            self.reserve(rows)

    def _rows(self, state):
        rows, s_stride = rows2(state, self.obs_dim, self.device, "state")
        if rows < 1 or rows > _actor_lib.POLICY_GRAD_MAX_ROWS:
            raise ValueError(f"uavx: FusedPolicyGrad takes 1..{_actor_lib.POLICY_GRAD_MAX_ROWS} rows, got {rows}")
        self._slots.fill_params(self.device)
        return rows, s_stride

    def _alpha(self, alpha):
        """(value, device pointer or None) for the ABI; SAC only."""
        if self.kind != _actor_lib.SAC:
            return 0.0, None
        if alpha_arg(alpha, self.device, "actor loss"):
            self._keep_alpha = alpha
            return 0.0, alpha.data_ptr()
        return float(alpha), None

    @torch.no_grad()
    def act(self, state, noise=None, generator=None):
        """Launch 1 alone: (action [B, 2], log_pi [B, 1] or None for TD3 / DDPG) of the live actor on `state` [B, 10] (any
        row stride), views of persistent buffers.  SAC: eps is `noise` ([B, 2], contiguous) or
        torch.randn((B, 2), generator=generator).  The activations stay in the workspace for backward_from."""
        rows, s_stride = self._rows(state)
        self._ready(rows)
        sac = self.kind == _actor_lib.SAC
        self._keep = noise = noise_arg(noise, rows, self.device, generator) if sac else None
        rc = self._lib.uavx_policy_grad_forward(
            self.kind, self.hidden1, self.hidden2, self._slots.pptrs, state.data_ptr(), rows, s_stride,
            noise.data_ptr() if sac else None, self._action.data_ptr(), self._logpi.data_ptr() if sac else None,
            self._ws.buf.data_ptr(), self._ws.buf.numel(), stream(self.device))
        _actor_lib.check(rc, "uavx_policy_grad_forward")
        self._acted = rows
        return self._action[:rows * 2].view(rows, 2), (self._logpi[:rows].view(rows, 1) if sac else None)

    @torch.no_grad()
    def backward_from(self, state, q, dqda, alpha=None):
        """Launches 3 to 5 alone, after act() on the same `state`: overwrites every actor parameter's .grad from the given
        q [T, B] and dq/da [T, B, 2] (contiguous float32, T the critic's tower count; SAC reads both towers, TD3 and DDPG
        the first) and returns the loss as a 0-d device tensor; SAC returns (loss, log_pi [B, 1])."""
        rows, s_stride = self._rows(state)
        T, dev = self._towers, self.device
        check_buffers(((q, (T, rows), "q"), (dqda, (T, rows, 2), "dqda")), dev)
        if self._acted != rows:
            raise RuntimeError(f"uavx: backward_from({rows} rows) needs act() on the same {rows} rows first (the workspace "
                               f"holds the activations of {self._acted})")
        a_val, a_ptr = self._alpha(alpha)
        gptrs = self._slots.fill_grads()
        sac = self.kind == _actor_lib.SAC
        rc = self._lib.uavx_policy_grad_backward(
            self.kind, self.hidden1, self.hidden2, self._slots.pptrs, state.data_ptr(), rows, s_stride, q.data_ptr(),
            dqda.data_ptr(), rows, a_val, a_ptr, gptrs, self._scalars.data_ptr(),
            self._scalars[1:].data_ptr() if sac else None, self._ws.buf.data_ptr(), self._ws.buf.numel(), stream(dev))
        _actor_lib.check(rc, "uavx_policy_grad_backward")
        if sac:
            return self._scalars[0], self._logpi[:rows].view(rows, 1)
        return self._scalars[0]

    def backward(self, state, alpha=None, noise=None, generator=None):
        """Sets every actor parameter's .grad to the gradient of the actor loss on `state` [B, 10] (overwritten, not
        accumulated) and returns the loss as a 0-d device tensor; SAC returns (loss, log_pi [B, 1]) and leaves
        log_pi_mean, so that the alpha update (sac.py:82) needs no second forward and no reduction.  SAC: alpha is a float or
        a 1-element float32 device tensor (read when the kernel runs); eps is `noise` ([B, 2]) or
        torch.randn((B, 2), generator=generator).  The results are views of persistent buffers, valid until the next call."""
        self._alpha(alpha)                             # checked before anything is launched
        action, _ = self.act(state, noise=noise, generator=generator)
        rows, T = action.shape[0], self._towers
        q, j = self._q[:T * rows].view(T, rows), self._j[:T * rows * 2].view(T, rows, 2)
        self.critic.q_dqda(state, action, towers=self._mask, out=(q, j))
        return self.backward_from(state, q, j, alpha=alpha)

    def close(self):
        """Releases the FusedActionGrad this block built (one passed in stays open)."""
        if self._owned is not None:
            self._owned.close()
            self._owned = None

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
from .fused_critic import _ACTOR_KINDS, _KIND_NAMES, FusedActionGrad, FusedCritic, _check_f32, _rows2, _stream
from .policy import DDPGCritic, TD3TwinQ, TwinQ

_CRITIC_KINDS = ((TwinQ, _actor_lib.SAC), (TD3TwinQ, _actor_lib.TD3), (DDPGCritic, _actor_lib.DDPG))


def _layers(actor, kind):
    if kind == _actor_lib.SAC:
        return (actor.linear1, actor.linear2, actor.mean_linear, actor.log_std_linear)
    if kind == _actor_lib.TD3:
        return (actor.l1, actor.l2, actor.l3)
    return (actor.input, actor.fc1, actor.fc2)


class FusedPolicyGrad:
    """actor: the live GaussianPolicy / TD3Actor / DDPGActor.  critic: a TwinQ / TD3TwinQ / DDPGCritic, an f32 FusedCritic
    or a FusedActionGrad.  Only the actor's parameters get a .grad: one that is usable (float32, contiguous, the
    parameter's shape and device) is overwritten in place, otherwise a persistent buffer is assigned; the critic's
    parameters' .grad is not touched."""

    def __init__(self, actor, critic):
        kind = next((k for cls, k in _ACTOR_KINDS if isinstance(actor, cls)), None)
        if kind is None:
            raise TypeError(f"uavx: FusedPolicyGrad takes a GaussianPolicy, TD3Actor or DDPGActor, not {type(actor).__name__}")
        # the pair and the devices are checked on the host, before anything touches a device
        cmod = critic.module if isinstance(critic, (FusedActionGrad, FusedCritic)) else critic
        ckind = next((k for cls, k in _CRITIC_KINDS if isinstance(cmod, cls)), None)
        if ckind is None:
            raise TypeError(f"uavx: FusedPolicyGrad takes a TwinQ, TD3TwinQ, DDPGCritic, FusedCritic or FusedActionGrad as "
                            f"its critic, not {type(critic).__name__}")
        if ckind != kind:
            raise TypeError(f"uavx: FusedPolicyGrad pairs a {_KIND_NAMES[kind]} actor ({type(actor).__name__}) with a "
                            f"{_KIND_NAMES[ckind]} critic ({type(cmod).__name__})")
        layers = _layers(actor, kind)
        w = layers[0].weight
        if w.device.type != "cuda":
            raise ValueError(f"uavx: FusedPolicyGrad needs the actor on a GPU (cuda:N), its parameters are on {w.device}")
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
        self._params = params
        self._towers = critic.critic.towers
        self._mask = 3 if kind == _actor_lib.SAC else 1
        dev = self.device
        # persistent .grad buffers, assigned to a parameter whose .grad is missing or unusable (no allocation per call)
        self._gbuf = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in params]
        self._scalars = torch.zeros(2, dtype=torch.float32, device=dev)      # loss, mean log_pi
        self._ws = torch.empty(0, dtype=torch.uint8, device=dev)
        self._cap = 0                                                        # rows the output buffers hold
        self._action = self._logpi = self._q = self._j = None
        self._acted = 0                                                      # rows of the forward the workspace holds
        self._keep = None
        self._pptrs = (ctypes.c_void_p * 8)()
        self._gptrs = (ctypes.c_void_p * 8)()
        # the sizes are checked now (a hidden size no kernel is compiled for raises here, not at the first call)
        self.workspace_bytes(1)

    @property
    def learner(self):
        return _KIND_NAMES[self.kind].lower()

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
        _actor_lib.check(rc, f"uavx_policy_grad_workspace_bytes({_KIND_NAMES[self.kind]}, {self.hidden1}, {self.hidden2}, "
                             f"{rows})")
        return n.value

    def reserve(self, rows):
        """Grows the workspace and the output buffers to what `rows` rows need (a graph capture cannot allocate them)."""
        rows = int(rows)
        need = self.workspace_bytes(rows)
        if self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
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
        if self._cap < rows or self._ws.numel() < self.workspace_bytes(rows):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"uavx: the workspace for {rows} rows must exist before a graph capture: call "
                                   f"reserve({rows}) first")
            self.reserve(rows)

    def _rows(self, state):
        rows, s_stride = _rows2(state, self.obs_dim, self.device, "state")
        if rows < 1 or rows > _actor_lib.POLICY_GRAD_MAX_ROWS:
            raise ValueError(f"uavx: FusedPolicyGrad takes 1..{_actor_lib.POLICY_GRAD_MAX_ROWS} rows, got {rows}")
        for i, p in enumerate(self._params):
            if p.dtype != torch.float32 or p.device != self.device or not p.is_contiguous():
                raise TypeError("uavx: FusedPolicyGrad reads contiguous float32 parameters on the actor's device")
            self._pptrs[i] = p.data_ptr()
        return rows, s_stride

    def _grads(self):
        out = []
        for p, buf in zip(self._params, self._gbuf):
            g = p.grad
            if (g is None or g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape
                    or not g.is_contiguous()):
                p.grad = g = buf
            out.append(g)
        return out

    def _alpha(self, alpha):
        """(value, device pointer or None) for the ABI; SAC only."""
        if self.kind != _actor_lib.SAC:
            return 0.0, None
        if alpha is None:
            raise ValueError("uavx: a SAC actor loss needs alpha (a float or a 1-element float32 device tensor)")
        if torch.is_tensor(alpha):
            _check_f32(alpha, self.device, "alpha")
            if alpha.numel() != 1:
                raise ValueError(f"uavx: alpha must have one element, got {tuple(alpha.shape)}")
            self._keep_alpha = alpha
            return 0.0, alpha.data_ptr()
        return float(alpha), None

    def _noise(self, rows, noise, generator):
        if self.kind != _actor_lib.SAC:
            return None
        if noise is None:
            return torch.randn((rows, 2), generator=generator, device=self.device, dtype=torch.float32)
        _check_f32(noise, self.device, "noise")
        if tuple(noise.shape) != (rows, 2):
            raise ValueError(f"uavx: noise must be [{rows}, 2], got {tuple(noise.shape)}")
        if not noise.is_contiguous():
            raise ValueError(f"uavx: noise must be a contiguous [{rows}, 2] tensor")
        return noise

    @torch.no_grad()
    def act(self, state, noise=None, generator=None):
        """Launch 1 alone: (action [B, 2], log_pi [B, 1] or None for TD3 / DDPG) of the live actor on `state` [B, 10] (any
        row stride), views of persistent buffers.  SAC: eps is `noise` ([B, 2], contiguous) or
        torch.randn((B, 2), generator=generator).  The activations stay in the workspace for backward_from."""
        rows, s_stride = self._rows(state)
        self._ready(rows)
        noise = self._noise(rows, noise, generator)
        self._keep = noise
        sac = self.kind == _actor_lib.SAC
        rc = self._lib.uavx_policy_grad_forward(
            self.kind, self.hidden1, self.hidden2, self._pptrs, state.data_ptr(), rows, s_stride,
            noise.data_ptr() if sac else None, self._action.data_ptr(), self._logpi.data_ptr() if sac else None,
            self._ws.data_ptr(), self._ws.numel(), _stream(self.device))
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
        for t, shape, what in ((q, (T, rows), "q"), (dqda, (T, rows, 2), "dqda")):
            _check_f32(t, dev, what)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"uavx: {what} must be a contiguous {list(shape)} tensor, got {tuple(t.shape)}")
        if self._acted != rows:
            raise RuntimeError(f"uavx: backward_from({rows} rows) needs act() on the same {rows} rows first (the workspace "
                               f"holds the activations of {self._acted})")
        a_val, a_ptr = self._alpha(alpha)
        for i, g in enumerate(self._grads()):
            self._gptrs[i] = g.data_ptr()
        sac = self.kind == _actor_lib.SAC
        rc = self._lib.uavx_policy_grad_backward(
            self.kind, self.hidden1, self.hidden2, self._pptrs, state.data_ptr(), rows, s_stride, q.data_ptr(),
            dqda.data_ptr(), rows, a_val, a_ptr, self._gptrs, self._scalars.data_ptr(),
            self._scalars[1:].data_ptr() if sac else None, self._ws.data_ptr(), self._ws.numel(), _stream(dev))
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

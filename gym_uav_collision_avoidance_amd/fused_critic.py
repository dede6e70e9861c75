"""FusedCritic and FusedTarget: the no-grad forward blocks of the reference's learners as ONE HIP launch each
(libuavx_actor.so, include/uavx_critic.h) instead of a chain of torch layers and element-wise kernels; FusedCriticLoss: the
gradient of the learners' critic loss in three launches (include/uavx_critic_grad.h), written into .grad; FusedActionGrad:
the critic towers of the learners' actor update, q and dq/da in one launch (include/uavx_action_grad.h); FusedActorLoss: the
actor-loss block built on it, the actor itself staying torch autograd.

    critic = FusedCritic.from_module(critic_target)                # TwinQ, TD3TwinQ or DDPGCritic
    q1, q2 = critic.q(state, action)                               # what the module's forward returns
    target = FusedTarget(actor_target, critic_target)              # the learner is told from the pair
    s, a, r, s2, m = mem.sample(256)
    y = target(s2, r, m, generator=g)                              # TD3's target_Q; SAC also takes alpha=

FusedTarget computes, in one launch, the block that opens each learner's update (the next action never leaves the chip):
    SAC   a', logπ = policy.sample(s')      y = r + mask·γ·(min(Q1', Q2')(s', a') − α·logπ)      (sac.py:56-60)
    TD3   a' = clamp(actor(s') + clamp(policy_noise·ε, ±noise_clip), ±1)   y = r + not_done·γ·min(Q1', Q2')(s', a')
    DDPG  a' = actor(s')                    y = r + γ·mask·Q'(s', a')                              (ddpg.py:62)
The packed weights are a SNAPSHOT taken at construction / refresh(): after an optimiser step or soft update the fused
networks keep computing with the old weights until refresh() is called.  Inputs must be float32 on the handle's device;
anything else raises (no conversion, no CPU path)."""
import ctypes

import torch

from . import _actor_lib
from ._fused_common import (KIND_NAMES, PRECISIONS, ParamSlots, Workspace, actor_layers, alpha_arg, check_buffers,
                            check_on_gpu, check_packable, column, critic_layers, noise_arg, pack_pointers, rows2,
                            stream)
from .fused_actor import FusedActor


class FusedCritic:
    def __init__(self, module, precision="f32"):
        found = critic_layers(module)
        if found is None:
            raise TypeError(f"uavx: FusedCritic takes a TwinQ, TD3TwinQ or DDPGCritic, not {type(module).__name__}")
        kind, layers = found
        device = check_packable(layers, precision, "FusedCritic")
        self.act_dim = 2
        self.obs_dim = layers[0].in_features - self.act_dim
        self.hidden1, self.hidden2 = layers[0].out_features, layers[1].out_features
        if len(layers) == 6 and tuple(l.weight.shape for l in layers[:3]) != tuple(l.weight.shape for l in layers[3:]):
            raise ValueError("uavx: the two towers of a twin critic must have the same shapes")
        self.module, self.kind, self.precision, self.device = module, kind, precision, device
        self.towers = 2 if len(layers) == 6 else 1
        self._layers = layers
        self._lib = _actor_lib.load()
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = self._lib.uavx_critic_create(kind, PRECISIONS[precision], self.obs_dim, self.hidden1, self.hidden2,
                                              self.act_dim, ctypes.byref(h))
        _actor_lib.check_critic(rc, f"uavx_critic_create({type(module).__name__}, {layers[0].in_features}->{self.hidden1}->"
                                    f"{self.hidden2}->1, {precision})")
        self._h = h
        self.refresh()

    @classmethod
    def from_module(cls, module, precision="f32"):
        """module: a TwinQ, TD3TwinQ or DDPGCritic (e.g. what policy.load_critic returns), float32, on a GPU."""
        return cls(module, precision)

    def refresh(self):
        """Re-packs the module's current parameters (one launch on the current stream)."""
        self._keep, ptrs = pack_pointers(self._layers, 12)
        _actor_lib.check_critic(self._lib.uavx_critic_pack(self._h, *ptrs, stream(self.device)), "uavx_critic_pack")
        return self

    def set_split_rows(self, rows):
        """Batches below `rows` run the small-batch variant (default _actor_lib.SPLIT_ROWS; 0 = never)."""
        _actor_lib.check_critic(self._lib.uavx_critic_set_split_rows(self._h, int(rows)), "uavx_critic_set_split_rows")
        return self

    @torch.no_grad()
    def q(self, state, action, out=None):
        """(q1, q2), each [B, 1], for a twin critic, q [B, 1] for DDPG: the module's forward on [B, 10] states and [B, 2]
        actions.  out: an optional float32 [B, 2] (twin) / [B, 1] tensor written in place; the results are views of it."""
        rows, s_stride = rows2(state, self.obs_dim, self.device, "state")
        arows, a_stride = rows2(action, self.act_dim, self.device, "action")
        if arows != rows:
            raise ValueError(f"uavx: state and action rows differ ({rows} vs {arows})")
        cols = self.towers
        if out is None:
            out = torch.empty((rows, cols), dtype=torch.float32, device=self.device)
        else:
            rows2(out, cols, self.device, "out")
            if out.shape[0] != rows:
                raise ValueError(f"uavx: out must be [{rows}, {cols}], got {tuple(out.shape)}")
        o_stride = out.stride(0) if rows > 1 else cols
        rc = self._lib.uavx_critic_q(self._h, state.data_ptr(), rows, s_stride, action.data_ptr(), a_stride, out.data_ptr(),
                                     o_stride, stream(self.device))
        _actor_lib.check_critic(rc, "uavx_critic_q")
        return (out[:, 0:1], out[:, 1:2]) if cols == 2 else out

    __call__ = q

    def close(self):
        if getattr(self, "_h", None):
            self._lib.uavx_critic_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def critic_handle(critic, who):
    """(FusedCritic, owned) for a block that takes a TwinQ / TD3TwinQ / DDPGCritic on a GPU or an open FusedCritic: the
    handle, and whether it was built here from the module, so that the block's close() releases it."""
    if isinstance(critic, FusedCritic):
        return critic, False
    if critic_layers(critic) is None:
        raise TypeError(f"uavx: {who} takes a TwinQ, TD3TwinQ, DDPGCritic or FusedCritic, not {type(critic).__name__}")
    check_on_gpu(next(critic.parameters()).device, who)
    return FusedCritic.from_module(critic), True


class FusedTarget:
    """The learner's TD target from a (next-action actor, target critic) pair: SAC (GaussianPolicy, TwinQ), TD3
    (TD3Actor, TD3TwinQ) or DDPG (DDPGActor, DDPGCritic).  actor / critic: modules or FusedActor / FusedCritic of the
    same precision.  gamma, policy_noise, noise_clip: the learners' defaults (sac.py gamma, td3.py:71-74)."""

    def __init__(self, actor, critic, precision="f32", gamma=0.99, policy_noise=0.2, noise_clip=0.5):
        self._owned = []
        if not isinstance(actor, FusedActor):
            actor = FusedActor.from_module(actor, precision)
            self._owned.append(actor)
        if not isinstance(critic, FusedCritic):
            critic = FusedCritic.from_module(critic, precision)
            self._owned.append(critic)
        if actor.kind != critic.kind:
            raise TypeError(f"uavx: FusedTarget pairs a {KIND_NAMES[actor.kind]} actor ({type(actor.module).__name__}) "
                            f"with a {KIND_NAMES[critic.kind]} critic ({type(critic.module).__name__})")
        if actor.precision != critic.precision:
            raise ValueError(f"uavx: actor ({actor.precision}) and critic ({critic.precision}) precisions differ")
        if actor.device != critic.device:
            raise ValueError(f"uavx: actor ({actor.device}) and critic ({critic.device}) are on different devices")
        self.actor, self.critic, self.kind = actor, critic, critic.kind
        self.precision, self.device = critic.precision, critic.device
        self.gamma, self.policy_noise, self.noise_clip = float(gamma), float(policy_noise), float(noise_clip)
        self._alpha = torch.zeros(1, dtype=torch.float32, device=self.device)   # holds a float alpha on the device

    @property
    def learner(self):
        return KIND_NAMES[self.kind].lower()

    def refresh(self):
        """Re-packs both networks (two launches on the current stream; capturable)."""
        self.actor.refresh()
        self.critic.refresh()
        return self

    def set_split_rows(self, rows):
        self.critic.set_split_rows(rows)
        return self

    @torch.no_grad()
    def __call__(self, next_state, reward, mask, alpha=None, generator=None, noise=None, out=None, aux=None):
        """y [B, 1] float32 (next_q_value / target_Q / y).  next_state [B, 10] (any row stride, e.g. a view of the replay
        ring); reward, mask [B] or [B, 1] with any row stride; alpha (SAC): a float or a 1-element float32 device tensor,
        read when the kernel runs; eps ~ torch.randn((B, 2), generator=generator) drawn as FusedActor.act draws it, or
        `noise` ([B, 2] float32) given; out: optional [B, 1] / [B] float32 written in place; aux: optional [B, 4] float32
        receiving a'0, a'1, logπ (0 unless SAC), min Q."""
        dev = self.device
        rows, s_stride = rows2(next_state, self.critic.obs_dim, dev, "next_state")
        r_stride = column(reward, rows, dev, "reward")
        m_stride = column(mask, rows, dev, "mask")
        if out is None:
            out = torch.empty((rows, 1), dtype=torch.float32, device=dev)
        o_stride = column(out, rows, dev, "out")
        a_ptr, a_stride = None, 4
        if aux is not None:
            arows, a_stride = rows2(aux, 4, dev, "aux")
            if arows != rows:
                raise ValueError(f"uavx: aux must be [{rows}, 4], got {tuple(aux.shape)}")
            a_ptr = aux.data_ptr()
        eps_ptr = None
        if self.kind != _actor_lib.DDPG:
            if noise is None:
                noise = torch.randn((rows, 2), generator=generator, device=dev, dtype=torch.float32)
            else:
                nrows, _ = rows2(noise, 2, dev, "noise")
                if nrows != rows or (rows > 1 and noise.stride(0) != 2):
                    raise ValueError(f"uavx: noise must be a contiguous [{rows}, 2] tensor")
            eps_ptr = noise.data_ptr()
        alpha_ptr = None
        if self.kind == _actor_lib.SAC:
            if alpha_arg(alpha, dev, "target"):
                alpha_ptr = alpha.data_ptr()
            else:
                self._alpha.fill_(float(alpha))
                alpha_ptr = self._alpha.data_ptr()
        self._keep = noise
        rc = self.critic._lib.uavx_critic_target(
            self.critic._h, self.actor._h, next_state.data_ptr(), rows, s_stride, reward.data_ptr(), r_stride,
            mask.data_ptr(), m_stride, eps_ptr, alpha_ptr, self.gamma, self.policy_noise, self.noise_clip, out.data_ptr(),
            o_stride, a_ptr, a_stride, stream(dev))
        _actor_lib.check_critic(rc, "uavx_critic_target")
        return out

    def close(self):
        """Releases the handles this target built from modules (a FusedActor / FusedCritic passed in stays open)."""
        for h in self._owned:
            h.close()
        self._owned = []


_LOSSES = {"mse": _actor_lib.GRAD_MSE, "l1": _actor_lib.GRAD_L1}
_DEFAULT_LOSS = {_actor_lib.SAC: "mse", _actor_lib.TD3: "mse", _actor_lib.DDPG: "l1"}


class FusedCriticLoss:
    """The gradient of the learners' critic loss (include/uavx_critic_grad.h, three HIP launches) written into the critic's
    .grad, in place of `zero_grad(); loss.backward()`; the optimiser step stays torch's:

        closs = FusedCriticLoss(critic)           # TwinQ / TD3TwinQ / DDPGCritic (f32, on a GPU) or an f32 FusedCritic
        l1, l2 = closs.backward(s, a, y)          # SAC / TD3: mse_loss(q1, y) + mse_loss(q2, y); DDPG: one L1 loss
        critic_optim.step()
        closs.reserve(rows)                       # sizes the workspace before a graph capture
        closs.backward(s, a, y, weight=w, q_out=q)   # prioritized replay: mean(w * loss) and q(s, a) [towers, B] (§24)

    loss: "mse" (sac.py, td3.py), "l1" (ddpg.py:68) or None for the learner's own.  The call reads the module's LIVE
    parameters when the kernels run (no refresh(): an optimiser step is seen by the next call), and leaves the packed
    snapshot of a FusedCritic untouched.  Inputs must be float32 on the module's device; anything else raises."""

    def __init__(self, critic, loss=None):
        # the loss is checked behind the critic's type and before its device, on the host
        found = critic_layers(critic.module if isinstance(critic, FusedCritic) else critic)
        if found is not None:
            loss = _DEFAULT_LOSS[found[0]] if loss is None else loss
            if loss not in _LOSSES:
                raise ValueError(f"uavx: loss must be one of {sorted(_LOSSES)} or None, not {loss!r}")
        fc, owned = critic_handle(critic, "FusedCriticLoss")
        self._owned = fc if owned else None
        self.critic, self.module, self.kind, self.device = fc, fc.module, fc.kind, fc.device
        self.loss = loss
        self._lib = fc._lib
        self._slots = ParamSlots((p for lin in fc._layers for p in (lin.weight, lin.bias)), 12, "FusedCriticLoss", "critic")
        self._loss = torch.zeros(fc.towers, dtype=torch.float32, device=self.device)
        self._ws = Workspace(self.device)

    def workspace_bytes(self, rows):
        n = ctypes.c_int64()
        rc = self._lib.uavx_critic_grad_workspace_bytes(self.critic._h, int(rows), ctypes.byref(n))
        _actor_lib.check_critic(rc, f"uavx_critic_grad_workspace_bytes({rows})")
        return n.value

    def reserve(self, rows):
        """Grows the workspace to what `rows` rows need (a graph capture cannot allocate it).  One workspace serves the
        unweighted and the weighted call: both lay it out by one plan."""
        self._ws.reserve(self.workspace_bytes(rows))
        return self

    def backward(self, state, action, y, weight=None, q_out=None):
        """Overwrites every critic parameter's .grad with the gradient of the loss on [B, 10] states, [B, 2] actions
        (any row stride) and targets y ([B] or [B, 1], any stride); returns the loss of each tower as 0-d device tensors
        (l1, l2), or the one loss of a DDPG critic.

        weight: per-row importance-sampling weights w ([B] or [B, 1] float32, any positive stride; finite and >= 0, which
        is not checked on the device): the loss becomes mean_b w_b (q - y)^2, or mean_b w_b |q - y|.  q_out: a contiguous
        [towers, B] float32 tensor that receives q(s, a) of the live critic, what a prioritized sampler's
        update_priorities takes.  With either given the call is uavx_wcritic_grad (include/uavx_wcritic_grad.h, the same
        three launches with the weighted row pass); weight=None there stands for a weight of 1, which gives the unweighted
        gradients bit for bit.  With both None the call is uavx_critic_grad."""
        dev = self.device
        rows, s_stride = rows2(state, self.critic.obs_dim, dev, "state")
        arows, a_stride = rows2(action, self.critic.act_dim, dev, "action")
        if arows != rows:
            raise ValueError(f"uavx: state and action rows differ ({rows} vs {arows})")
        y_stride = column(y, rows, dev, "y")
        if rows < 1 or rows > _actor_lib.GRAD_MAX_ROWS:
            raise ValueError(f"uavx: FusedCriticLoss takes 1..{_actor_lib.GRAD_MAX_ROWS} rows, got {rows}")
        weighted = weight is not None or q_out is not None
        w_ptr, w_stride, q_ptr = None, 1, None
        if weight is not None:
            w_stride = column(weight, rows, dev, "weight")
            if w_stride < 1:
                raise ValueError("uavx: weight must have a positive row stride")
            w_ptr = weight.data_ptr()
        if q_out is not None:
            check_buffers(((q_out, (self.critic.towers, rows), "q_out"),), dev)
            q_ptr = q_out.data_ptr()
        if weighted and self.critic.precision != "f32":
            raise RuntimeError(f"uavx: the weighted critic gradient has no kernel compiled for a "
                               f"{self.critic.precision} FusedCritic (f32 only)")
        pptrs = self._slots.fill_params(dev)
        self._ws.ensure(self.workspace_bytes(rows), rows)
        ws = self._ws.buf
        if not weighted:
            rc = self._lib.uavx_critic_grad(self.critic._h, _LOSSES[self.loss], pptrs, state.data_ptr(), rows, s_stride,
                                            action.data_ptr(), a_stride, y.data_ptr(), y_stride, self._slots.fill_grads(),
                                            self._loss.data_ptr(), ws.data_ptr(), ws.numel(), stream(dev))
            _actor_lib.check_critic(rc, "uavx_critic_grad")
        else:
            fc = self.critic
            with torch.cuda.device(dev):
                rc = self._lib.uavx_wcritic_grad(self.kind, fc.hidden1, fc.hidden2, fc.towers, _LOSSES[self.loss], pptrs,
                                                 state.data_ptr(), rows, s_stride, action.data_ptr(), a_stride,
                                                 y.data_ptr(), y_stride, w_ptr, w_stride, self._slots.fill_grads(),
                                                 self._loss.data_ptr(), q_ptr, ws.data_ptr(), ws.numel(), stream(dev))
            _actor_lib.check_wgrad(rc, "uavx_wcritic_grad")
        return (self._loss[0], self._loss[1]) if self.critic.towers == 2 else self._loss[0]

    def close(self):
        if self._owned is not None:
            self._owned.close()
            self._owned = None


class _ActionGradFn(torch.autograd.Function):
    """q of the selected towers as a function of the action: forward is the one launch and keeps J = dq/da, backward is
    sum_t g_t * J_t.  state and the critic's parameters are constants of the graph."""

    @staticmethod
    def forward(ctx, action, ag, state, mask):
        q, j = ag.q_dqda(state, action, towers=mask)
        ts = [t for t in range(ag.critic.towers) if mask >> t & 1]
        ctx.jac = [j[t] for t in ts]
        return tuple(q[t].unsqueeze(1) for t in ts)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gs):
        grad = gs[0] * ctx.jac[0]
        for g, j in zip(gs[1:], ctx.jac[1:]):
            grad = grad + g * j
        return grad, None, None, None


class FusedActionGrad:
    """The critic of the learners' actor update (sac.py:72, td3.py:144, ddpg.py:77), where it is only a differentiable
    function of the action: q_t(s, a) and the Jacobian dq_t/da of every selected tower in ONE HIP launch
    (include/uavx_action_grad.h), with no weight gradients:

        qa = FusedActionGrad(critic)              # TwinQ / TD3TwinQ / DDPGCritic (f32, on a GPU) or an f32 FusedCritic
        q1, q2 = qa(state, actor_output)          # differentiable in the action only; TD3: q1 = qa(s, a, towers=1)
        q, dqda = qa.q_dqda(state, action)        # [T, B] and [T, B, 2], no autograd

    towers: a bit mask (bit t selects tower t; None = all towers of the critic).  The call reads the module's LIVE
    parameters when the kernel runs (no refresh(): the critic's optimiser step before the actor update is seen), and leaves
    the packed snapshot of a FusedCritic untouched.  Inputs must be float32 on the module's device; anything else raises.

    How __call__ differs from running the module under autograd, as the reference does: its policy_loss.backward() also
    accumulates weight gradients into every critic parameter's .grad, which the trainers clear before they use them
    (sac.py:66 zero_grad, td3's critic_optimizer.zero_grad, ddpg.py:85-86) and which FusedCriticLoss overwrites.  Here
    the critic's parameters and `state` receive no gradient and their .grad is not touched."""

    def __init__(self, critic):
        fc, owned = critic_handle(critic, "FusedActionGrad")
        self._owned = fc if owned else None
        self.critic, self.module, self.kind, self.device = fc, fc.module, fc.kind, fc.device
        self._lib = fc._lib
        self._slots = ParamSlots((p for lin in fc._layers for p in (lin.weight, lin.bias)), 12, "FusedActionGrad", "critic",
                                 grads=False)

    def _mask(self, towers):
        full = (1 << self.critic.towers) - 1
        if towers is None:
            return full
        if isinstance(towers, bool) or not isinstance(towers, int):
            raise TypeError(f"uavx: towers must be an int bit mask or None, not {type(towers).__name__}")
        if towers < 1 or towers & ~full:
            raise ValueError(f"uavx: towers mask {towers} selects nothing or a tower this {KIND_NAMES[self.kind]} critic "
                             f"({self.critic.towers} tower(s)) does not have")
        return towers

    @torch.no_grad()
    def q_dqda(self, state, action, towers=None, out=None):
        """(q [T, B], dqda [T, B, 2]) for T = the critic's tower count, on [B, 10] states and [B, 2] actions (any row
        stride).  Only the selected towers' entries are written: the others keep what `out` held (without `out` they are
        uninitialised).  out = (q, dqda): preallocated contiguous float32 buffers, e.g. for a graph capture."""
        dev, T = self.device, self.critic.towers
        mask = self._mask(towers)
        rows, s_stride = rows2(state, self.critic.obs_dim, dev, "state")
        arows, a_stride = rows2(action, self.critic.act_dim, dev, "action")
        if arows != rows:
            raise ValueError(f"uavx: state and action rows differ ({rows} vs {arows})")
        if rows < 1 or rows > _actor_lib.ACTION_GRAD_MAX_ROWS:
            raise ValueError(f"uavx: FusedActionGrad takes 1..{_actor_lib.ACTION_GRAD_MAX_ROWS} rows, got {rows}")
        pptrs = self._slots.fill_params(dev)
        if out is None:
            q = torch.empty((T, rows), dtype=torch.float32, device=dev)
            j = torch.empty((T, rows, 2), dtype=torch.float32, device=dev)
        else:
            q, j = out
            check_buffers(((q, (T, rows), "out[0]"), (j, (T, rows, 2), "out[1]")), dev)
        rc = self._lib.uavx_action_grad(self.critic._h, mask, pptrs, state.data_ptr(), rows, s_stride,
                                        action.data_ptr(), a_stride, q.data_ptr(), j.data_ptr(), stream(dev))
        _actor_lib.check_critic(rc, "uavx_action_grad")
        return q, j

    def __call__(self, state, action, towers=None):
        """What the module's forward returns, differentiable in `action` only: (q1, q2), each [B, 1], for a twin critic
        (one of them alone under towers=1 or 2), q [B, 1] for DDPG."""
        mask = self._mask(towers)
        qs = _ActionGradFn.apply(action, self, state, mask)
        return qs if len(qs) == 2 else qs[0]

    def close(self):
        if self._owned is not None:
            self._owned.close()
            self._owned = None


class FusedActorLoss:
    """The learners' actor-loss block, `zero_grad(); loss.backward()` of
        SAC   (alpha * log_pi - min(Q1, Q2)(s, pi(s))).mean()      (model.py:88-99, sac.py:70-78)
        TD3   -Q1(s, actor(s)).mean()                              (td3.py:144)
        DDPG  -Q(s, actor(s)).mean()                               (ddpg.py:77-79)
    with the critic towers in one HIP launch (FusedActionGrad) and the actor's own forward and backward torch autograd on
    the live module; the optimiser step stays the caller's (FusedAdam or torch):

        aloss = FusedActorLoss(actor, critic)     # the learner is told from the pair, as FusedTarget does
        loss, log_pi = aloss.backward(s, alpha=alpha, generator=g)      # SAC; TD3 / DDPG: loss = aloss.backward(s)
        actor_optim.step()

    actor: the live GaussianPolicy / TD3Actor / DDPGActor.  critic: a TwinQ / TD3TwinQ / DDPGCritic, an f32 FusedCritic or
    a FusedActionGrad."""

    def __init__(self, actor, critic):
        found = actor_layers(actor)
        if found is None:
            raise TypeError(f"uavx: FusedActorLoss takes a GaussianPolicy, TD3Actor or DDPGActor, not {type(actor).__name__}")
        kind = found[0]
        self._owned = None
        if not isinstance(critic, FusedActionGrad):
            critic = self._owned = FusedActionGrad(critic)
        if critic.kind != kind:
            raise TypeError(f"uavx: FusedActorLoss pairs a {KIND_NAMES[kind]} actor ({type(actor).__name__}) with a "
                            f"{KIND_NAMES[critic.kind]} critic ({type(critic.module).__name__})")
        params = list(actor.parameters())
        for p in params:
            if p.device != critic.device or p.dtype != torch.float32:
                raise ValueError(f"uavx: FusedActorLoss needs the actor in float32 on the critic's device {critic.device}, "
                                 f"a parameter is {p.dtype} on {p.device}")
        self.actor, self.critic, self.kind, self.device = actor, critic, kind, critic.device
        self._params = params

    @property
    def learner(self):
        return KIND_NAMES[self.kind].lower()

    def backward(self, state, alpha=None, noise=None, generator=None):
        """Sets every actor parameter's .grad to the gradient of the actor loss on `state` [B, 10] (cleared first, not
        accumulated) and returns the loss as a 0-d device tensor; SAC returns (loss, log_pi.detach() [B, 1]) so that the
        alpha update (sac.py:82) needs no second forward.  SAC: alpha is a float or a device tensor; eps is `noise`
        ([B, 2]) or torch.randn((B, 2), generator=generator)."""
        dev = self.device
        rows, _ = rows2(state, self.critic.critic.obs_dim, dev, "state")
        if rows < 1 or rows > _actor_lib.ACTION_GRAD_MAX_ROWS:
            raise ValueError(f"uavx: FusedActorLoss takes 1..{_actor_lib.ACTION_GRAD_MAX_ROWS} rows, got {rows}")
        if self.kind == _actor_lib.SAC:
            alpha_arg(alpha, dev, "actor loss", one_element=False)
            noise = noise_arg(noise, rows, dev, generator, contiguous=False)
        for p in self._params:
            p.grad = None
        with torch.enable_grad():
            if self.kind == _actor_lib.SAC:
                mean, log_std = self.actor(state)
                std = log_std.exp()
                normal = torch.distributions.Normal(mean, std, validate_args=False)   # validation would synchronise
                x_t = mean + std * noise                                               # normal.rsample()
                y_t = torch.tanh(x_t)                                                  # action_scale 1, action_bias 0
                log_prob = normal.log_prob(x_t)
                log_prob = log_prob - torch.log(1.0 * (1 - y_t.pow(2)) + 1e-6)
                log_pi = log_prob.sum(1, keepdim=True)
                q1, q2 = self.critic(state, y_t)
                loss = ((alpha * log_pi) - torch.min(q1, q2)).mean()
            elif self.kind == _actor_lib.TD3:
                loss = -self.critic(state, self.actor(state), towers=1).mean()
            else:
                loss = -self.critic(state, self.actor(state)).mean()
            loss.backward()
        if self.kind == _actor_lib.SAC:
            return loss.detach(), log_pi.detach()
        return loss.detach()

    def close(self):
        """Releases the FusedActionGrad this block built (one passed in stays open)."""
        if self._owned is not None:
            self._owned.close()
            self._owned = None

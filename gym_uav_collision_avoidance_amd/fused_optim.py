"""FusedAdam and soft_update: the optimiser step and the soft target update that close each learner's update, as
multi-tensor HIP launches (libuavx_actor.so, include/uavx_optim.h) instead of torch's per-tensor kernels.

    opt = FusedAdam(critic_optim, target=critic_target, tau=5e-3)      # wraps the learner's torch.optim.Adam
    closs.backward(s, a, y)
    opt.step(update_target=True, refresh=target)                       # Adam + soft update (2 launches) + the re-pack
    soft_update(actor_target, actor, tau)                              # TD3's delayed update, one launch

FusedAdam keeps the optimiser's state where torch keeps it (optim.state[p]["exp_avg"], ["exp_avg_sq"],
["max_exp_avg_sq"]), so optim.state_dict() stays the reference's checkpoint format and a checkpoint loaded with
load_state_dict continues under the fused step.  Only the step COUNT lives elsewhere while training runs: in a device
int64 the kernels read and advance, which is what lets a captured graph take a new step on every replay.  sync_state()
writes it back into every state[p]["step"] (one host synchronisation, outside the update loop); state_dict() on the wrapper
does that first; reload() reads it again after the wrapped optimiser's own load_state_dict.

lr, betas, eps and tau are read from the param group at every call; a captured graph keeps the values of its capture.

    opt = FusedAdam(critic_optim, target=critic_target, max_grad_norm=10.0)      # clips the global gradient norm first

With max_grad_norm the step goes through libuavx_clip.so (include/uavx_clip.h) instead: one norm over every
gradient of every param group, as torch.nn.utils.clip_grad_norm_(all_params, max_norm), then the same Adam arithmetic on
g·coef; three launches for one group.  .grad itself is NOT rewritten: opt.clip_coef is what to multiply it by.  The bound
lives in a device slot (set_max_grad_norm), so a captured step follows it.  Without the keyword nothing differs and the
library is not even loaded.
There is NO fallback: anything the kernels do not implement raises before a launch."""
import ctypes
import math
import numbers

import torch

from . import _actor_lib
from ._fused_common import stream
from .fused_actor import FusedActor
from .fused_critic import FusedCritic, FusedTarget

_MAXT = _actor_lib.OPTIM_MAX_TENSORS


def _params_of(x, what):
    if isinstance(x, torch.nn.Module):
        return list(x.parameters())
    try:
        ps = list(x)
    except TypeError:
        raise TypeError(f"uavx: {what} must be a module or an iterable of tensors, not {type(x).__name__}") from None
    for p in ps:
        if not torch.is_tensor(p):
            raise TypeError(f"uavx: {what} must hold tensors, found {type(p).__name__}")
    return ps


def _check_shapes(targets, params, what):
    if len(targets) != len(params):
        raise ValueError(f"uavx: {what} has {len(targets)} parameters, the other side {len(params)}")
    for i, (t, p) in enumerate(zip(targets, params)):
        if t.shape != p.shape:
            raise ValueError(f"uavx: {what} parameter {i} is {tuple(t.shape)}, its counterpart {tuple(p.shape)}")


def _check_tensor(t, device, what):
    """contiguous, non-empty float32 on a GPU (`device`, or any when None) -> its device."""
    if t.dtype != torch.float32:
        raise TypeError(f"uavx: {what} must be float32, got {t.dtype}")
    if t.device.type != "cuda":
        raise ValueError(f"uavx: {what} must be on a GPU (cuda:N), it is on {t.device}: there is no CPU path")
    if device is not None and t.device != device:
        raise ValueError(f"uavx: {what} is on {t.device}, the others on {device}")
    if not t.is_contiguous():
        raise ValueError(f"uavx: {what} must be contiguous")
    if t.numel() < 1:
        raise ValueError(f"uavx: {what} is empty")
    return t.device


def check_max_grad_norm(x, what="max_grad_norm"):
    """A clip bound as a float: a finite number > 0 that is still finite and > 0 as a float32 (tensors are refused: the bound
    is written into a device slot by the host)."""
    ok = isinstance(x, numbers.Real) and not isinstance(x, bool)
    if ok:
        f32 = float(torch.tensor(float(x), dtype=torch.float32))
        ok = math.isfinite(float(x)) and x > 0 and math.isfinite(f32) and f32 > 0
    if not ok:
        raise ValueError(f"uavx: {what} must be a finite float > 0 (or None: no clipping), got {x!r}")
    return float(x)


def _check_tau(tau):
    tau = float(tau)
    if not 0.0 <= tau <= 1.0:
        raise ValueError(f"uavx: tau must be in [0, 1], got {tau}")
    return tau


class _Table:
    """ctypes arrays of one call, allocated once."""

    def __init__(self, n, columns):
        self.n = n
        self.numel = (ctypes.c_int64 * _MAXT)()
        self.cols = {c: (ctypes.c_void_p * _MAXT)() for c in columns}

    def fill(self, column, tensors):
        arr = self.cols[column]
        for i, t in enumerate(tensors):
            arr[i] = None if t is None else t.data_ptr()
        return arr


def soft_update(target, source, tau):
    """target ← target·(1 − tau) + source·tau over every parameter pair (sac.py / ddpg.py soft_update, td3.py:152-156; the
    same float32 bits as either spelling), one launch per 16 tensors on the current stream.  target, source: modules or
    iterables of tensors, contiguous float32 on one GPU, equal in number and shapes."""
    ts, ss = _params_of(target, "target"), _params_of(source, "source")
    _check_shapes(ts, ss, "target")
    tau = _check_tau(tau)
    if not ts:
        raise ValueError("uavx: soft_update got no parameters")
    dev = None
    for i, (t, s) in enumerate(zip(ts, ss)):
        dev = _check_tensor(t, dev, f"target parameter {i}")
        _check_tensor(s, dev, f"source parameter {i}")
    lib = _actor_lib.load()
    with torch.cuda.device(dev):
        for k in range(0, len(ts), _MAXT):
            tab = _Table(len(ts[k:k + _MAXT]), ("t", "s"))
            for i, t in enumerate(ts[k:k + _MAXT]):
                tab.numel[i] = t.numel()
            rc = lib.uavx_optim_soft_update(tab.n, tab.fill("t", ts[k:k + _MAXT]), tab.fill("s", ss[k:k + _MAXT]), tab.numel,
                                            tau, stream(dev))
            _actor_lib.check(rc, "uavx_optim_soft_update")


class FusedAdam:
    """torch.optim.Adam's step (AMSGrad included) over each param group in two HIP launches, optionally with the soft update
    of a target network and the re-pack of a fused handle behind it.

    optimizer: a torch.optim.Adam (not AdamW) with weight_decay = 0, maximize = False, differentiable = False and a float
    lr; its parameters contiguous float32 on one GPU, at most 16 per group.  target: the target network (module or
    parameters, in the optimiser's parameter order), tau: its soft-update rate.

    max_grad_norm: None (the default: the step above, nothing else), or a finite float > 0: every step first clips the
    global gradient norm -- ONE norm over all parameters of all param groups, float64 sums in a fixed order -- to it, as
    torch.nn.utils.clip_grad_norm_ would, in three launches for one group.  The parameters' .grad is read
    and NOT rewritten: the step uses g * clip_coef.  grad_norm, clip_coef (0-d float32) and clipped_steps (0-d int64) are
    device views of the last step's record; reading them synchronises, holding them does not.  record: with max_grad_norm,
    an 8-byte aligned float32 device tensor of 6 elements to keep that record in (norm, coef, the int64 count, the bound),
    for a caller that reads it in one copy with data of its own; None allocates one."""

    def __init__(self, optimizer, target=None, tau=5e-3, max_grad_norm=None, record=None):
        if type(optimizer) is not torch.optim.Adam:
            raise TypeError(f"uavx: FusedAdam wraps a torch.optim.Adam, not {type(optimizer).__name__}")
        self.max_grad_norm = None if max_grad_norm is None else check_max_grad_norm(max_grad_norm)
        self.optimizer = optimizer
        self.tau = _check_tau(tau)
        self._groups = [list(g["params"]) for g in optimizer.param_groups]
        for gi, g in enumerate(optimizer.param_groups):
            self._hyper(g)
            if not 1 <= len(g["params"]) <= _MAXT:
                raise ValueError(f"uavx: param group {gi} has {len(g['params'])} tensors, FusedAdam takes 1..{_MAXT} "
                                 f"per group")
        flat = [p for ps in self._groups for p in ps]
        self._targets = None
        if target is not None:
            ts = _params_of(target, "target")
            _check_shapes(ts, flat, "target")
            it = iter(ts)
            self._targets = [[next(it) for _ in ps] for ps in self._groups]
        dev = None
        for i, p in enumerate(flat):
            dev = _check_tensor(p, dev, f"parameter {i}")
        for i, t in enumerate(ts if target is not None else ()):
            _check_tensor(t, dev, f"target parameter {i}")
        self.device = dev
        self._lib = _actor_lib.load()
        self._tabs = [_Table(len(ps), ("p", "g", "m", "v", "x", "t")) for ps in self._groups]
        for tab, ps in zip(self._tabs, self._groups):
            for i, p in enumerate(ps):
                tab.numel[i] = p.numel()
        # per group: the step count the kernels advance, and the slot of the prologue's two scalars
        self._steps = torch.zeros(len(self._groups), dtype=torch.int64, device=dev)
        self._scalars = torch.zeros((len(self._groups), 2), dtype=torch.float32, device=dev)
        self._step_ptr, self._scalar_ptr = self._steps.data_ptr(), self._scalars.data_ptr()
        self._clip = None
        if self.max_grad_norm is not None:
            self._setup_clip(record)
        elif record is not None:
            raise ValueError("uavx: record goes with max_grad_norm: this FusedAdam does not clip")
        self.reload()

    def _setup_clip(self, record):
        """Loads libuavx_clip.so and allocates what a clipped step reads and writes besides the optimiser's state: the
        record with the slot of the bound behind it (one 24-byte allocation, or `record`) and the workspace of per-block
        sums (8 bytes per 1024 gradient elements: sized here, so a capture needs no reserve())."""
        from . import _clip_lib
        if len(self._groups) > _clip_lib.MAX_GROUPS:
            raise ValueError(f"uavx: FusedAdam clips over 1..{_clip_lib.MAX_GROUPS} param groups, got {len(self._groups)}")
        self._clip = _clip_lib
        self._clip_lib = _clip_lib.load()
        dev = self.device
        # norm, coef | clipped (int64) | max_norm, padding
        if record is None:
            record = torch.zeros(6, dtype=torch.float32, device=dev)
        elif (not torch.is_tensor(record) or record.dtype != torch.float32 or tuple(record.shape) != (6,)
                or record.device != dev or not record.is_contiguous() or record.data_ptr() % 8):
            raise ValueError(f"uavx: record must be a contiguous float32 tensor of 6 elements on {dev}, 8-byte aligned")
        self._clip_rec = record.zero_()
        self.grad_norm, self.clip_coef = self._clip_rec[0], self._clip_rec[1]
        self.clipped_steps = self._clip_rec[2:4].view(torch.int64)[0]
        self._clip_rec[1] = 1.0
        self._clip_rec[4] = self.max_grad_norm
        self._clip_groups = (_clip_lib.Group * len(self._groups))()
        for gi, (cg, tab) in enumerate(zip(self._clip_groups, self._tabs)):
            cg.n, cg.numel = tab.n, ctypes.addressof(tab.numel)
            cg.step, cg.scalars = self._step_ptr + 8 * gi, self._scalar_ptr + 8 * gi
        need = ctypes.c_int64()
        _clip_lib.check(self._clip_lib.uavx_clip_workspace_bytes(len(self._groups), self._clip_groups, ctypes.byref(need)),
                        "uavx_clip_workspace_bytes")
        self._clip_work = torch.empty(need.value // 8, dtype=torch.float64, device=dev)

    def set_max_grad_norm(self, max_grad_norm):
        """Moves the bound of an object built with max_grad_norm: written into the device slot on the current stream, so
        the next step -- a replay of a captured one included -- clips to it."""
        if self._clip is None:
            raise ValueError("uavx: set_max_grad_norm needs a FusedAdam built with max_grad_norm: this one does not clip")
        self.max_grad_norm = check_max_grad_norm(max_grad_norm)
        self._clip_rec[4] = self.max_grad_norm
        return self

    @staticmethod
    def _hyper(g):
        """(lr, beta1, beta2, eps) of a param group, refusing what the kernels do not implement."""
        if torch.is_tensor(g["lr"]):
            raise TypeError("uavx: FusedAdam takes a float lr, not a tensor")
        if g.get("weight_decay", 0) != 0:
            raise ValueError(f"uavx: FusedAdam does not implement weight_decay (got {g['weight_decay']})")
        if g.get("maximize", False):
            raise ValueError("uavx: FusedAdam does not implement maximize=True")
        if g.get("differentiable", False):
            raise ValueError("uavx: FusedAdam does not implement differentiable=True")
        b1, b2 = g["betas"]
        if torch.is_tensor(b1) or torch.is_tensor(b2):
            raise TypeError("uavx: FusedAdam takes float betas, not tensors")
        return float(g["lr"]), float(b1), float(b2), float(g["eps"])

    @property
    def param_groups(self):
        return self.optimizer.param_groups

    def hyper(self, group=0):
        """(lr, beta1, beta2, eps) of a param group as the next step would read them (raises on what is not implemented)."""
        return self._hyper(self.optimizer.param_groups[group])

    def step_pointer(self, group=0):
        """Device address of the int64 step count of a param group, for a kernel that takes the group's step itself."""
        return self._step_ptr + 8 * group

    def zero_grad(self, set_to_none=True):
        self.optimizer.zero_grad(set_to_none=set_to_none)

    def _new_step(self, p, g):
        """A zero step count as torch.optim.Adam creates it for this group."""
        dtype = torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32
        if g.get("capturable", False) or g.get("fused", False):
            return torch.zeros((), dtype=dtype, device=p.device)
        return torch.tensor(0.0, dtype=dtype)

    def reload(self):
        """Adopts the wrapped optimiser's state: creates what is missing (zeros, as torch's first step does), checks what
        is there and copies the step count to the device.  Call it after optimizer.load_state_dict()."""
        steps = []
        for gi, (g, ps) in enumerate(zip(self.optimizer.param_groups, self._groups)):
            if len(g["params"]) != len(ps) or any(a is not b for a, b in zip(g["params"], ps)):
                raise RuntimeError("uavx: the optimiser's parameters changed after FusedAdam wrapped it")
            keys = ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if g["amsgrad"] else ())
            seen = set()
            for i, p in enumerate(ps):
                st = self.optimizer.state[p]
                if "step" not in st:
                    st["step"] = self._new_step(p, g)
                for k in keys:
                    if k not in st:
                        st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    s = st[k]
                    _check_tensor(s, self.device, f"state {k!r} of parameter {i} in group {gi}")
                    if s.shape != p.shape:
                        raise ValueError(f"uavx: state {k!r} of parameter {i} in group {gi} is {tuple(s.shape)}, the "
                                         f"parameter {tuple(p.shape)}")
                seen.add(float(st["step"]))
            if len(seen) != 1:
                raise ValueError(f"uavx: the parameters of group {gi} are at different steps {sorted(seen)}; FusedAdam "
                                 f"keeps one count per group")
            t = seen.pop()
            if t < 0 or t != int(t):
                raise ValueError(f"uavx: group {gi} has a step count of {t}")
            steps.append(int(t))
        self._steps.copy_(torch.tensor(steps, dtype=torch.int64))
        return self

    def sync_state(self):
        """Writes the device step counts into every state[p]["step"], in the dtype and on the device torch keeps it (one
        device-to-host copy: keep it out of the update loop)."""
        for g, ps, t in zip(self.optimizer.param_groups, self._groups, self._steps.tolist()):
            for p in ps:
                st = self.optimizer.state[p]
                if torch.is_tensor(st.get("step")):
                    st["step"].fill_(t)
                else:
                    st["step"] = self._new_step(p, g).fill_(t)
        return self

    def state_dict(self):
        return self.sync_state().optimizer.state_dict()

    def load_state_dict(self, state_dict):
        self.optimizer.load_state_dict(state_dict)
        self.reload()

    def step(self, update_target=False, refresh=None):
        """One Adam step of every group from the parameters' .grad.  update_target: also soft-update the target given at
        construction, from the new parameters, in the same launch.  refresh: a FusedTarget, FusedCritic or FusedActor
        whose refresh() (its existing pack launches) is enqueued behind the step on the same stream."""
        if update_target and self._targets is None:
            raise ValueError("uavx: step(update_target=True) needs the target given to FusedAdam(...)")
        if refresh is not None and not isinstance(refresh, (FusedTarget, FusedCritic, FusedActor)):
            raise TypeError(f"uavx: refresh must be a FusedTarget, FusedCritic or FusedActor, not {type(refresh).__name__}")
        dev = self.device
        calls = []
        for gi, (g, ps, tab) in enumerate(zip(self.optimizer.param_groups, self._groups, self._tabs)):
            hyper = self._hyper(g)
            grads = []
            for i, p in enumerate(ps):
                gr = p.grad
                if gr is None:
                    raise ValueError(f"uavx: parameter {i} of group {gi} has no .grad")
                if (gr.dtype != torch.float32 or gr.device != dev or gr.shape != p.shape or not gr.is_contiguous()
                        or gr.is_sparse):
                    raise ValueError(f"uavx: .grad of parameter {i} of group {gi} must be a contiguous float32 "
                                     f"{tuple(p.shape)} on {dev}")
                if not p.is_contiguous() or p.device != dev or p.dtype != torch.float32:
                    raise ValueError(f"uavx: parameter {i} of group {gi} is no longer contiguous float32 on {dev}")
                grads.append(gr)
            sts = [self.optimizer.state[p] for p in ps]
            calls.append((gi, tab, hyper, tab.fill("p", ps), tab.fill("g", grads),
                          tab.fill("m", [s["exp_avg"] for s in sts]), tab.fill("v", [s["exp_avg_sq"] for s in sts]),
                          tab.fill("x", [s["max_exp_avg_sq"] for s in sts]) if g["amsgrad"] else None,
                          tab.fill("t", self._targets[gi]) if update_target else None))
        st = stream(dev)
        if self._clip is not None:
            for cg, (gi, tab, (lr, b1, b2, eps), p, g, m, v, x, t) in zip(self._clip_groups, calls):
                cg.params, cg.grads, cg.exp_avg, cg.exp_avg_sq = (ctypes.addressof(c) for c in (p, g, m, v))
                cg.max_exp_avg_sq = None if x is None else ctypes.addressof(x)
                cg.targets = None if t is None else ctypes.addressof(t)
                cg.lr, cg.beta1, cg.beta2, cg.eps, cg.tau = lr, b1, b2, eps, self.tau
            with torch.cuda.device(dev):
                rc = self._clip_lib.uavx_clip_step(len(calls), self._clip_groups, self._clip_work.data_ptr(),
                                                   self._clip_work.numel() * 8, self._clip_rec.data_ptr() + 16,
                                                   self._clip_rec.data_ptr(), st)
            self._clip.check(rc, "uavx_clip_step")
            if refresh is not None:
                refresh.refresh()
            return
        with torch.cuda.device(dev):
            for gi, tab, (lr, b1, b2, eps), p, g, m, v, x, t in calls:
                rc = self._lib.uavx_optim_adam(tab.n, p, g, m, v, x, t, tab.numel, lr, b1, b2, eps, self.tau,
                                               self._step_ptr + 8 * gi, self._scalar_ptr + 8 * gi, st)
                _actor_lib.check(rc, "uavx_optim_adam")
        if refresh is not None:
            refresh.refresh()

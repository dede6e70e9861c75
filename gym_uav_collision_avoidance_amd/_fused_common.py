"""What the bindings of libuavx_actor.so share: the stream lookup, the argument checks, the learner kind
and layers of a policy.py module, the `.grad` slots and the workspace of the gradient units.  Plain functions and two small
classes; every check raises before a launch and converts nothing."""
import ctypes

import torch

from . import _actor_lib
from .policy import DDPGActor, DDPGCritic, GaussianPolicy, TD3Actor, TD3TwinQ, TwinQ

PRECISIONS = {"f32": _actor_lib.F32, "bf16": _actor_lib.BF16}
KIND_NAMES = {_actor_lib.SAC: "SAC", _actor_lib.TD3: "TD3", _actor_lib.DDPG: "DDPG"}


def stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def check_f32(t, device, what):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != device:
        raise TypeError(f"uavx: {what} must be a float32 tensor on {device}, got {getattr(t, 'dtype', type(t))} on "
                        f"{getattr(t, 'device', 'host')}")


def rows2(t, cols, device, what, unit_stride=True):
    """t [B, cols] float32 on device, with unit last stride unless unit_stride=False -> (B, row stride)."""
    check_f32(t, device, what)
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError(f"uavx: {what} must be [B, {cols}], got {tuple(t.shape)}")
    rows = t.shape[0]
    if unit_stride and rows and t.stride(1) != 1:
        raise ValueError(f"uavx: {what} must have unit stride along its last dimension")
    return rows, (t.stride(0) if rows > 1 else cols)


def column(t, rows, device, what):
    """t [B] or [B, 1] float32 on device, any row stride -> row stride."""
    check_f32(t, device, what)
    if tuple(t.shape) not in ((rows,), (rows, 1)):
        raise ValueError(f"uavx: {what} must be [{rows}] or [{rows}, 1], got {tuple(t.shape)}")
    return t.stride(0) if rows > 1 else 1


def check_buffers(pairs, device):
    """Each (tensor, shape, name) of `pairs`: a contiguous float32 tensor of that shape on device."""
    for t, shape, what in pairs:
        check_f32(t, device, what)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"uavx: {what} must be a contiguous {list(shape)} tensor, got {tuple(t.shape)}")


def alpha_arg(alpha, device, who, one_element=True):
    """SAC's temperature as the `who` block takes it: a float, or a float32 tensor on device (of one element, unless
    one_element=False) that the kernels read when they run -> whether it is a tensor."""
    if alpha is None:
        raise ValueError(f"uavx: a SAC {who} needs alpha (a float or a {'1-element float32 ' if one_element else ''}"
                         f"device tensor)")
    if not torch.is_tensor(alpha):
        return False
    check_f32(alpha, device, "alpha")
    if one_element and alpha.numel() != 1:
        raise ValueError(f"uavx: alpha must have one element, got {tuple(alpha.shape)}")
    return True


def noise_arg(noise, rows, device, generator=None, contiguous=True):
    """eps [rows, 2] of a SAC actor loss: `noise` checked, or torch.randn((rows, 2), generator=generator) drawn as
    FusedActor.act draws it."""
    if noise is None:
        return torch.randn((rows, 2), generator=generator, device=device, dtype=torch.float32)
    check_f32(noise, device, "noise")
    if tuple(noise.shape) != (rows, 2):
        raise ValueError(f"uavx: noise must be [{rows}, 2], got {tuple(noise.shape)}")
    if contiguous and not noise.is_contiguous():
        raise ValueError(f"uavx: noise must be a contiguous [{rows}, 2] tensor")
    return noise


def actor_layers(module):
    """(learner kind, the nn.Linear layers in the kernels' order) of a policy.py actor, or None for anything else."""
    if isinstance(module, GaussianPolicy):
        return _actor_lib.SAC, (module.linear1, module.linear2, module.mean_linear, module.log_std_linear)
    if isinstance(module, TD3Actor):
        return _actor_lib.TD3, (module.l1, module.l2, module.l3)
    if isinstance(module, DDPGActor):
        return _actor_lib.DDPG, (module.input, module.fc1, module.fc2)
    return None


def critic_layers(module):
    """(learner kind, the nn.Linear layers, tower by tower) of a policy.py critic, or None for anything else."""
    if isinstance(module, TwinQ):
        return _actor_lib.SAC, (module.linear1, module.linear2, module.linear3, module.linear4, module.linear5,
                                module.linear6)
    if isinstance(module, TD3TwinQ):
        return _actor_lib.TD3, (module.l1, module.l2, module.l3, module.l4, module.l5, module.l6)
    if isinstance(module, DDPGCritic):
        return _actor_lib.DDPG, (module.input, module.fc1, module.fc2)
    return None


def check_on_gpu(device, who, what="module"):
    if device.type != "cuda":
        raise ValueError(f"uavx: {who} needs the {what} on a GPU (cuda:N), its parameters are on {device}")


def check_packable(layers, precision, who):
    """What FusedActor and FusedCritic ask of the layers they pack: a known precision, a GPU, float32 -> the device."""
    if precision not in PRECISIONS:
        raise ValueError(f"uavx: precision must be one of {sorted(PRECISIONS)}, not {precision!r}")
    w = layers[0].weight
    check_on_gpu(w.device, who)
    for lin in layers:
        if lin.weight.dtype != torch.float32 or lin.bias is None or lin.bias.dtype != torch.float32:
            raise TypeError(f"uavx: {who} packs float32 parameters; keep the module in float32 and pick "
                            "precision='bf16' for the bf16 kernel")
    return w.device


def pack_pointers(layers, slots):
    """(tensors to keep alive, `slots` pointers: weight and bias of each layer, then NULLs) for a pack launch."""
    keep = [p.detach().contiguous() for lin in layers for p in (lin.weight, lin.bias)]
    return keep, [p.data_ptr() for p in keep] + [None] * (slots - len(keep))


def capture_guard(what, rows):
    """Refuses to grow `what` while the current stream is being captured: a graph capture cannot allocate."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"uavx: the {what} for {rows} rows must exist before a graph capture: call reserve({rows}) "
                           f"first")


class Workspace:
    """The uint8 scratch tensor a unit hands to its kernels (`buf`), grown on demand and never shrunk."""

    def __init__(self, device):
        self.buf = torch.empty(0, dtype=torch.uint8, device=device)

    def reserve(self, need):
        """Grows to `need` bytes -> whether the tensor was replaced (what the old one held is gone)."""
        if self.buf.numel() >= need:
            return False
        self.buf = torch.empty(need, dtype=torch.uint8, device=self.buf.device)
        return True

    def ensure(self, need, rows):
        """reserve() from a call on `rows` rows: raises instead of growing during a graph capture."""
        if self.buf.numel() < need:
            capture_guard("workspace", rows)
            self.reserve(need)


class ParamSlots:
    """The live parameters of one network as the gradient kernels take them: a ctypes table of their addresses and, with
    grads=True, one of their `.grad` tensors, both allocated once and refilled by every call."""

    def __init__(self, params, slots, who, where, grads=True):
        self.params = list(params)
        self.pptrs = (ctypes.c_void_p * slots)()
        self._refusal = f"uavx: {who} reads contiguous float32 parameters on the {where}'s device"
        if grads:
            # persistent .grad buffers, assigned to a parameter whose .grad is missing or unusable (no allocation per call)
            self.gbuf = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
            self.gptrs = (ctypes.c_void_p * slots)()

    def fill_params(self, device):
        pptrs, f32 = self.pptrs, torch.float32
        for i, p in enumerate(self.params):
            if p.dtype != f32 or p.device != device or not p.is_contiguous():
                raise TypeError(self._refusal)
            pptrs[i] = p.data_ptr()
        return pptrs

    def fill_grads(self):
        """Every parameter's .grad becomes one the kernels can overwrite in place: its own if usable, else the buffer."""
        gptrs, f32 = self.gptrs, torch.float32
        for i, (p, buf) in enumerate(zip(self.params, self.gbuf)):
            g = p.grad
            if g is None or g.dtype != f32 or g.device != p.device or g.shape != p.shape or not g.is_contiguous():
                p.grad = g = buf
            gptrs[i] = g.data_ptr()
        return gptrs

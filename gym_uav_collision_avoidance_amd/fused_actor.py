"""FusedActor: the whole forward of a policy.py actor (GaussianPolicy / TD3Actor / DDPGActor) as ONE HIP launch
(libuavx_actor.so, include/uavx_actor.h) instead of three GEMMs and separate activation kernels.

    actor = FusedActor.from_module(policy, precision="f32")      # or "bf16": bf16 operands, f32 accumulation
    actor.act(mem.state, out=mem.action_slot())                   # writes the replay ring's action slot in place
    mem.step(polar=True)

The packed weights are a SNAPSHOT taken by from_module() / refresh(): after the module's parameters change (an optimiser
step, load_state_dict) the fused actor keeps computing with the old ones until refresh() is called.
Inputs must be float32 on the actor's device; anything else raises (no conversion, no CPU path)."""
import ctypes

import torch

from . import _actor_lib
from ._fused_common import PRECISIONS, actor_layers, check_packable, pack_pointers, stream


class FusedActor:
    def __init__(self, module, precision="f32"):
        found = actor_layers(module)
        if found is None:
            raise TypeError(f"uavx: FusedActor takes a GaussianPolicy, TD3Actor or DDPGActor, not {type(module).__name__}")
        kind, layers = found
        device = check_packable(layers, precision, "FusedActor")
        self.module, self.kind, self.precision, self.device = module, kind, precision, device
        self._layers = layers
        self._lib = _actor_lib.load()
        self.obs_dim, self.hidden1 = layers[0].in_features, layers[0].out_features
        self.hidden2, self.act_dim = layers[1].out_features, layers[2].out_features
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = self._lib.uavx_actor_create(kind, PRECISIONS[precision], self.obs_dim, self.hidden1, self.hidden2,
                                             self.act_dim, ctypes.byref(h))
        _actor_lib.check(rc, f"uavx_actor_create({type(module).__name__}, {self.obs_dim}->{self.hidden1}->{self.hidden2}->"
                             f"{self.act_dim}, {precision})")
        self._h = h
        self.refresh()

    @classmethod
    def from_module(cls, module, precision="f32"):
        """module: a GaussianPolicy, TD3Actor or DDPGActor (e.g. what policy.load_actor returns), float32, on a GPU."""
        return cls(module, precision)

    def _stream(self):
        """stream(self.device).  Not called in this tree: kept for code written against the method, such as the earlier
        tests/test_gpu_explore.py, which has to keep passing against this package."""
        return stream(self.device)

    def refresh(self):
        """Re-packs the module's current parameters (one launch on the current stream)."""
        self._keep, ptrs = pack_pointers(self._layers, 8)   # contiguous() copies live until the next pack
        _actor_lib.check(self._lib.uavx_actor_pack(self._h, *ptrs, stream(self.device)), "uavx_actor_pack")
        return self

    def _rows(self, obs):
        if not torch.is_tensor(obs) or obs.dtype != torch.float32 or obs.device != self.device:
            raise TypeError(f"uavx: FusedActor needs float32 observations on {self.device}, got "
                            f"{getattr(obs, 'dtype', type(obs))} on {getattr(obs, 'device', 'host')}")
        if obs.shape[-1] != self.obs_dim:
            raise ValueError(f"uavx: observations must be [..., {self.obs_dim}], got {tuple(obs.shape)}")
        lead = tuple(obs.shape[:-1])
        o2 = obs.reshape(-1, self.obs_dim)
        if o2.numel() and o2.stride(1) != 1:
            o2 = o2.contiguous()
        return lead, o2

    def _out(self, out, lead, cols):
        if out is None:
            return torch.empty(lead + (cols,), dtype=torch.float32, device=self.device)
        if out.dtype != torch.float32 or out.device != self.device or tuple(out.shape) != lead + (cols,):
            raise ValueError(f"uavx: out must be float32 {lead + (cols,)} on {self.device}, got {out.dtype} "
                             f"{tuple(out.shape)} on {out.device}")
        return out

    def _launch(self, o2, eps, scale, mode, out, cols):
        rows = o2.shape[0]
        try:
            d2 = out.view(rows, cols)
        except RuntimeError:
            raise ValueError("uavx: out must be viewable as [rows, columns] with one row stride (written in place)") from None
        if rows and d2.stride(1) != 1:
            raise ValueError("uavx: out must have unit stride along its last dimension")
        obs_stride = o2.stride(0) if rows > 1 else self.obs_dim
        out_stride = d2.stride(0) if rows > 1 else cols
        rc = self._lib.uavx_actor_forward(self._h, o2.data_ptr(), rows, obs_stride, None if eps is None else eps.data_ptr(),
                                          float(scale), mode, d2.data_ptr(), out_stride, stream(self.device))
        _actor_lib.check(rc, "uavx_actor_forward")
        return out

    @torch.no_grad()
    def raw(self, obs):
        """Pre-tanh heads: (mean, clamped log_std) for SAC, the pre-tanh output for TD3 / DDPG."""
        lead, o2 = self._rows(obs)
        cols = 4 if self.kind == _actor_lib.SAC else 2
        y = self._launch(o2, None, 0.0, _actor_lib.RAW, self._out(None, lead, cols), cols)
        return (y[..., :2], y[..., 2:]) if self.kind == _actor_lib.SAC else y

    @torch.no_grad()
    def act(self, obs, evaluate=True, generator=None, noise_std=0.1, noise=None, out=None):
        """The wrapped module's act(): SAC tanh(mean) / tanh(mean + exp(log_std) * eps); TD3 a / clamp(a + noise_std * eps);
        DDPG a / clamp(a + noise).  eps = torch.randn(shape, generator=generator) drawn exactly as policy.py draws it, so
        the same generator state gives the same noise.  out: a float32 [..., 2] tensor (e.g. DeviceReplay.action_slot())
        written in place and returned."""
        lead, o2 = self._rows(obs)
        out = self._out(out, lead, 2)
        shape = lead + (2,)
        eps, scale, mode = None, 0.0, _actor_lib.DETERMINISTIC
        if self.kind == _actor_lib.DDPG:
            if not evaluate and noise is not None:
                eps = torch.as_tensor(noise, device=self.device).to(torch.float32).expand(shape).contiguous()
                scale, mode = 1.0, _actor_lib.ADD_CLAMP
        elif not evaluate:
            eps = torch.randn(shape, generator=generator, device=self.device, dtype=torch.float32)
            if self.kind == _actor_lib.SAC:
                mode = _actor_lib.SAC_SAMPLE
            else:
                scale, mode = noise_std, _actor_lib.ADD_CLAMP
        return self._launch(o2, eps, scale, mode, out, 2)

    __call__ = act

    def close(self):
        if getattr(self, "_h", None):
            self._lib.uavx_actor_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

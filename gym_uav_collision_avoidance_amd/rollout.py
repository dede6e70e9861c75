"""The on-policy side of the device ring: GAE(λ) advantages and returns over the last steps of a DeviceReplay, computed where
the rollout lies (include/uavx_gae.h, libuavx_gae.so).

A DeviceReplay already is a rollout buffer -- time-major, written zero-copy by the step launch.  What an on-policy learner
needs on top is the backward recurrence in time that turns rewards and value estimates into advantages, cut and bootstrapped
by the ring's own rules (an agent's done, the env's episode end, re-initialisation rows, the ring's wrap).  In torch that is
a group of launches per step of the rollout; here it is one launch, three with the normalisation.  There is NO fallback: a
missing library or device raises."""
import collections
import ctypes
import math

import torch

Advantages = collections.namedtuple("Advantages", "adv ret valid adv_norm")
Stats = collections.namedtuple("Stats", "n mean std")


def _unit(name, x):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or math.isnan(x) or not 0.0 <= x <= 1.0:
        raise ValueError(f"uavx: RolloutAdvantages: {name} must be a float in [0, 1], got {x!r}")
    return float(x)


class RolloutAdvantages:
    def __init__(self, mem, gamma=0.99, lam=0.95, normalize=True):
        """mem: a DeviceReplay (packed flags or not; its num_learners is respected).  gamma, lam: in [0, 1].
        normalize: also produce adv_norm = (adv − mean) / (std + 1e-8) over the window's valid entries."""
        self.gamma, self.lam = _unit("gamma", gamma), _unit("lam", lam)
        self.mem, self.normalize = mem, bool(normalize)
        self.shape = (mem.L, mem.env.num_envs, mem.env.num_agents)
        dev = mem.rew.device
        self.outputs = Advantages(torch.zeros(self.shape, dtype=torch.float32, device=dev),
                               torch.zeros(self.shape, dtype=torch.float32, device=dev),
                               torch.zeros(self.shape, dtype=torch.uint8, device=dev),
                               torch.zeros(self.shape, dtype=torch.float32, device=dev) if self.normalize else None)
        self._record = torch.zeros(3, dtype=torch.float64, device=dev)       # uavx_gae_stats: int64 n, double mean, std
        self.stats = Stats(self._record[:1].view(torch.int64)[0], self._record[1], self._record[2])
        self._lib = self._ring = self._work = self._other = None

    def _steps(self, steps):
        count, T = self.mem.count, self.mem.T
        if count < 1:
            raise ValueError("uavx: RolloutAdvantages: the ring holds no step yet")
        if steps is None:
            return min(count, T)
        if isinstance(steps, bool) or not isinstance(steps, int) or not 1 <= steps <= min(count, T):
            raise ValueError(f"uavx: RolloutAdvantages: steps must be an int in [1, min(count, T)] = [1, {min(count, T)}], "
                             f"got {steps!r}")
        return steps

    def window(self, steps=None):
        """The slots of the window's steps, oldest first, as an int64 device tensor: index the ring (and the tensors
        compute() returns) with it."""
        steps = self._steps(steps)
        k = torch.arange(self.mem.count - steps, self.mem.count, dtype=torch.int64, device=self.mem.rew.device)
        return k % self.mem.L

    def _bind(self):
        from . import _gae_lib
        mem = self.mem
        if mem.rew.device.type != "cuda":
            raise ValueError("uavx: RolloutAdvantages computes on a GPU: there is no CPU path")
        self._gae = _gae_lib
        self._lib = _gae_lib.load()
        L, E, N = self.shape
        skip, ended = (None, None) if mem.packed else (mem.skip.data_ptr(), mem.ended.data_ptr())
        self._ring = _gae_lib.Ring(rew=mem.rew.data_ptr(), done=mem.done.data_ptr(), skip=skip, ended=ended, slots=L, envs=E,
                                   agents=N, learners=mem.num_learners)
        need = ctypes.c_int64(0)
        _gae_lib.check(self._lib.uavx_gae_workspace_bytes(ctypes.byref(self._ring), ctypes.byref(need)),
                       "uavx_gae_workspace_bytes")
        self._work = torch.zeros(max(1, need.value // 8), dtype=torch.float64, device=mem.rew.device)

    def _ring_with(self, rewards):
        """The ring struct with `rewards` in place of mem.rew (kept: the same tensor comes again every update)."""
        if self._other is None or self._other.rew != rewards.data_ptr():
            r = self._ring
            self._other = self._gae.Ring(rew=rewards.data_ptr(), done=r.done, skip=r.skip, ended=r.ended, slots=r.slots,
                                         envs=r.envs, agents=r.agents, learners=r.learners)
        return self._other

    def compute(self, values, steps=None, rewards=None):
        """values: contiguous [L, E, N] float32 device tensor, the caller's V of the observation in every slot of the ring.
        rewards: None, or a contiguous [L, E, N] float32 tensor on the ring's device that is read in place of mem.rew
        (normalize.RolloutNormalizer.rewards()).
        Returns Advantages(adv, ret, valid, adv_norm): preallocated [L, E, N] tensors written in the window's rows only
        (window(steps) gathers them), valid until the next call; adv_norm is None without normalize.  The record (n, mean,
        std as 0-d device tensors) is left in .stats.  Enqueued on the current stream; nothing is read on the host."""
        steps = self._steps(steps)
        if not torch.is_tensor(values) or values.dtype != torch.float32 or tuple(values.shape) != self.shape:
            got = f"{values.dtype} {tuple(values.shape)}" if torch.is_tensor(values) else type(values).__name__
            raise ValueError(f"uavx: RolloutAdvantages: values must be float32 {self.shape}, got {got}")
        if values.device != self.mem.rew.device or not values.is_contiguous():
            raise ValueError("uavx: RolloutAdvantages: values must be contiguous and on the ring's device")
        if rewards is not None:
            if not torch.is_tensor(rewards) or rewards.dtype != torch.float32 or tuple(rewards.shape) != self.shape:
                got = f"{rewards.dtype} {tuple(rewards.shape)}" if torch.is_tensor(rewards) else type(rewards).__name__
                raise ValueError(f"uavx: RolloutAdvantages: rewards must be float32 {self.shape}, got {got}")
            if rewards.device != self.mem.rew.device or not rewards.is_contiguous():
                raise ValueError("uavx: RolloutAdvantages: rewards must be contiguous and on the ring's device")
        if self._lib is None:
            self._bind()
        o = self.outputs
        ring = self._ring if rewards is None else self._ring_with(rewards)
        with torch.cuda.device(values.device):
            rc = self._lib.uavx_gae_compute(ctypes.byref(ring), values.data_ptr(), self.mem.count, steps, self.gamma,
                                            self.lam, o.adv.data_ptr(), o.ret.data_ptr(), o.valid.data_ptr(),
                                            o.adv_norm.data_ptr() if self.normalize else None,
                                            self._record.data_ptr(), self._work.data_ptr(), self._work.numel() * 8,
                                            torch.cuda.current_stream(values.device).cuda_stream)
        self._gae.check(rc, "uavx_gae_compute")
        return o

"""Running observation and return normalisation over the device ring (include/uavx_norm.h, libuavx_norm.so):
what VecNormalize and NormalizeReward keep, computed where the rollout lies.

    norm = RolloutNormalizer(mem, gamma=0.99)
    x = norm.obs(mem.state)                 # [..., F] normalised with the CURRENT record; nothing is folded
    xs, rs = norm.obs_ring(), norm.rewards()   # every slot of mem.obs normalised, mem.rew scaled (preallocated)
    norm.fold_returns(); norm.fold_obs()    # fold the steps since the last fold into the record

The record (count, mean and M2 per observation feature; the same for the discounted returns) lives in device memory and is
only ever touched by the library: a fold is two float64 passes over the ring's sample rows in a fixed order and Chan's merge,
three launches; applying it is one.  Which rows are samples is PPO's rule (learner columns, no re-initialisation rows, no rows
of an agent parked in an env that went on).  Nothing here reads the device from the host.  There is NO fallback: a missing
library or device raises."""
import collections
import ctypes
import math

import torch

NormStats = collections.namedtuple("NormStats", "n_obs mean var n_ret var_ret")

_RECORD_WORDS, _MAX_FEATURES, _BLOCK = 36, 16, 256       # uavx_norm_record in 8-byte words; UAVX_NORM_MAX_FEATURES, _BLOCK
_MEAN, _M2, _N_RET, _M2_RET = 1, 17, 33, 35              # where its fields start


def _unit(name, x):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or math.isnan(x) or not 0.0 <= x <= 1.0:
        raise ValueError(f"uavx: RolloutNormalizer: {name} must be a float in [0, 1], got {x!r}")
    return float(x)


def _finite(name, x, positive):
    ok = not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x) and (x > 0 if positive else x >= 0)
    if not ok:
        raise ValueError(f"uavx: RolloutNormalizer: {name} must be a finite float {'> 0' if positive else '>= 0'}, got {x!r}")
    return float(x)


class RolloutNormalizer:
    def __init__(self, mem, gamma=0.99, obs=True, reward=True, clip_obs=10.0, clip_reward=10.0, eps=1e-8):
        """mem: a DeviceReplay (packed flags or not; its num_learners is respected).  gamma: the discount of the return
        whose variance scales the rewards, in [0, 1].  obs, reward: which of the two statistics are kept; the calls of the
        other raise.  clip_obs, clip_reward: the clamp of the normalised values.  eps: added to the variance under the root.
        Each fold keeps its own counter of the steps it has folded; both start at the oldest step the ring still holds."""
        for name, x in (("obs", obs), ("reward", reward)):
            if not isinstance(x, bool):
                raise ValueError(f"uavx: RolloutNormalizer: {name} must be a bool, got {x!r}")
        self.gamma = _unit("gamma", gamma)
        self.clip_obs, self.clip_reward = _finite("clip_obs", clip_obs, True), _finite("clip_reward", clip_reward, True)
        self.eps = _finite("eps", eps, False)
        self.mem, self.keeps_obs, self.keeps_reward = mem, obs, reward
        L, E, N = self.shape = (mem.L, mem.env.num_envs, mem.env.num_agents)
        self.features = F = int(mem.obs.shape[-1])
        if tuple(mem.obs.shape) != (L, E, N, F) or not 1 <= F <= _MAX_FEATURES:
            raise ValueError(f"uavx: RolloutNormalizer: the ring's observations must be [L, E, N, F] with 1 <= F <= "
                             f"{_MAX_FEATURES}, got {tuple(mem.obs.shape)}")
        dev = mem.rew.device
        self._record = torch.zeros(_RECORD_WORDS, dtype=torch.float64, device=dev)
        self.carry = torch.zeros((E, N), dtype=torch.float64, device=dev)
        self._work = torch.zeros((2 * F + 1) * (-(-E * N // _BLOCK)), dtype=torch.float64, device=dev)
        self._obs_ring = torch.zeros((L, E, N, F), dtype=torch.float32, device=dev) if obs else None
        self._rew_ring = torch.zeros((L, E, N), dtype=torch.float32, device=dev) if reward else None
        self.folded_obs = self.folded_ret = max(0, mem.count - mem.T)
        self._lib = self._ring = None

    # -- the record ----------------------------------------------------------------------------------------------------------
    @property
    def stats(self):
        """NormStats(n_obs, mean [F], var [F], n_ret, var_ret) as device tensors: the counts are views of the record, the
        variances M2 / n (1 while n = 0) formed by torch on the device.  Nothing is read on the host."""
        r, F = self._record, self.features
        n_obs, n_ret = r[:1].view(torch.int64)[0], r[_N_RET:_N_RET + 1].view(torch.int64)[0]
        var = torch.where(n_obs > 0, r[_M2:_M2 + F] / n_obs.to(torch.float64), torch.ones_like(r[_M2:_M2 + F]))
        var_ret = torch.where(n_ret > 0, r[_M2_RET] / n_ret.to(torch.float64), torch.ones_like(r[_M2_RET]))
        return NormStats(n_obs, r[_MEAN:_MEAN + F], var, n_ret, var_ret)

    def _bind(self):
        mem = self.mem
        if mem.rew.device.type != "cuda":
            raise ValueError("uavx: RolloutNormalizer computes on a GPU: there is no CPU path")
        from . import _norm_lib
        self._norm = _norm_lib
        self._lib = _norm_lib.load()
        L, E, N = self.shape
        skip, ended = (None, None) if mem.packed else (mem.skip.data_ptr(), mem.ended.data_ptr())
        self._ring = _norm_lib.Ring(rew=mem.rew.data_ptr(), done=mem.done.data_ptr(), skip=skip, ended=ended, slots=L, envs=E,
                                    agents=N, learners=mem.num_learners)
        need = ctypes.c_int64(0)
        _norm_lib.check(self._lib.uavx_norm_workspace_bytes(ctypes.byref(self._ring), self.features, ctypes.byref(need)),
                        "uavx_norm_workspace_bytes")
        if need.value != self._work.numel() * 8:
            raise RuntimeError(f"uavx: RolloutNormalizer sized its workspace at {self._work.numel() * 8} bytes, the library "
                               f"asks for {need.value}")

    def _call(self, name, *args):
        if self._lib is None:
            self._bind()
        dev = self.mem.rew.device
        with torch.cuda.device(dev):
            rc = getattr(self._lib, name)(*args, torch.cuda.current_stream(dev).cuda_stream)
        self._norm.check(rc, name)

    # -- folding -------------------------------------------------------------------------------------------------------------
    def _window(self, what, switch, folded):
        if not switch:
            raise ValueError(f"uavx: RolloutNormalizer: this normalizer keeps no {what} statistics")
        count, T = self.mem.count, self.mem.T
        if count - folded > T:
            raise ValueError(f"uavx: RolloutNormalizer: {count - folded} steps are not folded into the {what} statistics yet, "
                             f"the ring keeps {T}: the older rows were overwritten")
        return folded, count

    def fold_obs(self):
        """Folds the observations of the sample rows of the steps [folded_obs, mem.count) into the record."""
        first, count = self._window("observation", self.keeps_obs, self.folded_obs)
        if count > first:
            self._call("uavx_norm_fold_obs", ctypes.byref(self._ring_struct()), self.mem.obs.data_ptr(), self.features, first,
                       count, self._record.data_ptr(), self._work.data_ptr(), self._work.numel() * 8)
            self.folded_obs = count

    def fold_returns(self):
        """Walks the discounted return R = r + γ·C forwards over the steps [folded_ret, mem.count), from the carry the last
        fold left, and folds R of the sample rows into the record."""
        first, count = self._window("return", self.keeps_reward, self.folded_ret)
        if count > first:
            self._call("uavx_norm_fold_returns", ctypes.byref(self._ring_struct()), first, count, self.gamma,
                       self.carry.data_ptr(), self._record.data_ptr(), self._work.data_ptr(), self._work.numel() * 8)
            self.folded_ret = count

    def _ring_struct(self):
        if self._lib is None:
            self._bind()
        return self._ring

    # -- applying ------------------------------------------------------------------------------------------------------------
    def obs(self, x, out=None):
        """x: contiguous [..., F] float32 on the ring's device -> (x − mean) / sqrt(var + eps) clamped to ±clip_obs, with the
        record as it stands when the launch runs.  out: a tensor like x (x itself is fine); default a new one."""
        if not self.keeps_obs:
            raise ValueError("uavx: RolloutNormalizer: this normalizer keeps no observation statistics")
        F = self.features
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() < 1 or x.shape[-1] != F:
            got = f"{x.dtype} {tuple(x.shape)}" if torch.is_tensor(x) else type(x).__name__
            raise ValueError(f"uavx: RolloutNormalizer: observations must be float32 [..., {F}], got {got}")
        if x.device != self.mem.rew.device or not x.is_contiguous():
            raise ValueError("uavx: RolloutNormalizer: observations must be contiguous and on the ring's device")
        if out is None:
            out = torch.empty_like(x)
        elif (not torch.is_tensor(out) or out.dtype != torch.float32 or out.shape != x.shape or out.device != x.device
              or not out.is_contiguous()):
            raise ValueError("uavx: RolloutNormalizer: out must be a contiguous float32 tensor of the observations' shape on "
                             "their device")
        if x.numel():                     # an empty tensor has no address to hand over
            self._call("uavx_norm_apply_obs", self._record.data_ptr(), x.data_ptr(), out.data_ptr(), x.numel() // F, F,
                       self.eps, self.clip_obs)
        return out

    def obs_ring(self):
        """[L, E, N, F]: every slot of mem.obs normalised, in a preallocated tensor valid until the next call."""
        if not self.keeps_obs:
            raise ValueError("uavx: RolloutNormalizer: this normalizer keeps no observation statistics")
        return self.obs(self.mem.obs, out=self._obs_ring)

    def rewards(self):
        """[L, E, N]: mem.rew / sqrt(var_ret + eps) clamped to ±clip_reward, in a preallocated tensor valid until the next
        call.  The mean is not subtracted."""
        if not self.keeps_reward:
            raise ValueError("uavx: RolloutNormalizer: this normalizer keeps no return statistics")
        self._call("uavx_norm_scale_rewards", self._record.data_ptr(), self.mem.rew.data_ptr(), self._rew_ring.data_ptr(),
                   self.mem.rew.numel(), self.eps, self.clip_reward)
        return self._rew_ring

    # -- snapshot / restore (checkpoint.py) ---------------------------------------------------------------------
    def state_dict(self):
        """Tensors and built-in types only: the record, the carry, the two counters and what the normalizer keeps."""
        return {"kind": "rollout_normalizer", "record": self._record, "carry": self.carry, "features": int(self.features),
                "obs": self.keeps_obs, "reward": self.keeps_reward, "folded_obs": int(self.folded_obs),
                "folded_ret": int(self.folded_ret)}

    def check_state(self, sd):
        """Raises ValueError unless sd is a state_dict() of a normalizer that keeps the same statistics over a ring of the
        same shape."""
        if not isinstance(sd, dict) or sd.get("kind") != "rollout_normalizer":
            raise ValueError("uavx: RolloutNormalizer.load_state_dict was given the state of something else")
        for name, mine in (("features", self.features), ("obs", self.keeps_obs), ("reward", self.keeps_reward)):
            if type(sd.get(name)) is not type(mine) or sd[name] != mine:
                raise ValueError(f"uavx: the saved normalizer has {name} = {sd.get(name)!r}, this one {name} = {mine!r}")
        for name, mine in (("record", self._record), ("carry", self.carry)):
            t = sd.get(name)
            if not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != tuple(mine.shape):
                raise ValueError(f"uavx: the saved normalizer's {name!r} does not fit this ring")
        for name in ("folded_obs", "folded_ret"):
            if isinstance(sd.get(name), bool) or not isinstance(sd.get(name), int) or sd[name] < 0:
                raise ValueError(f"uavx: the saved normalizer has {name} = {sd.get(name)!r}, not a step count")

    def load_state_dict(self, sd):
        """Restores a state_dict() in place; what check_state() refuses is refused before a byte is written."""
        self.check_state(sd)
        self._record.copy_(sd["record"])
        self.carry.copy_(sd["carry"])
        self.folded_obs, self.folded_ret = sd["folded_obs"], sd["folded_ret"]
        return self

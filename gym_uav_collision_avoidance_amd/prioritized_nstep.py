"""Prioritized n-step replay (libuavx_keywalk.so, include/uavx_keywalk.h): the n-step walk of §22 started
from the keys a prioritized sample (§23) returned.

    per = PrioritizedNStepSampler(mem, alpha=0.6, beta=0.4, n_step=3, gamma=0.99)
    s, a, R, s_n, m, w, key = per.sample(256, generator=g)  # R = sum_{j<len} gamma^j r_j, s_n the observation len steps on,
                                                            # m = (1 - done_last) * gamma^(len-1); w, key as the parent's
    ..., tr, en = per.sample(256, with_flags=True)          # the flags of the last row walked
    ..., length = per.sample(256, with_length=True)         # len per row, uint8 in 1..n_step (0: key -1), behind the flags
    per.update_priorities(key, q, y)                        # inherited: the keys name the START rows

    walk = KeyWalk(mem, n_step=3, gamma=0.99)               # the launch alone
    walk.extend(key, reward, next_state, mask)              # overwrites the three (and flags / length when given) in place

A sample is PrioritizedReplaySampler's own -- ONE torch.rand((rows,)), the refresh, the draw with its one-step gather --
followed by ONE more launch that reads each row's key and overwrites reward, next_state and mask (and the flags) with the
n-step values.  The search of the draw lives in libuavx_prio.so, whose source is pinned, and is not copied.  A row whose
key is -1 (nothing to draw) or no longer in the ring's window keeps what the draw wrote and gets length 0.  n_step = 1
reproduces PrioritizedReplaySampler bit for bit.
There is NO fallback: anything the kernels do not implement raises before a launch and before the generator moves."""
import ctypes
import math

import torch

from . import _keywalk_lib, _lib
from ._fused_common import stream
from .fused_replay import FusedReplaySampler
from .fused_replay_nstep import check_n_step
from .prioritized_replay import PrioritizedReplaySampler
from .replay import DeviceReplay

_MAX_ROWS = _keywalk_lib.MAX_ROWS


def check_walk(n_step, gamma, who="KeyWalk"):
    """n_step in 1..8 (check_n_step's range) and a finite gamma in [0, 1] as (int, float), refused otherwise."""
    n, _ = check_n_step(n_step, 0.0, who)
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        g = float("nan")
    if not (math.isfinite(g) and 0.0 <= g <= 1.0):
        raise ValueError(f"uavx: {who} takes a finite gamma in [0, 1], got {gamma!r}")
    return n, g


class KeyWalk:
    """uavx_keywalk on a DeviceReplay: the n-step walk from given keys, one launch."""

    def __init__(self, mem, n_step=3, gamma=0.99):
        if not isinstance(mem, DeviceReplay):
            raise TypeError(f"uavx: KeyWalk takes a DeviceReplay, not {type(mem).__name__}")
        self.mem = mem
        self.device = mem.obs.device
        if self.device.type != "cuda":
            raise ValueError(f"uavx: KeyWalk needs the ring on a GPU (cuda:N), it is on {self.device}: there is no CPU path")
        self.n_step, self.gamma = check_walk(n_step, gamma)
        self._lib = _keywalk_lib.load()
        self._ring = _keywalk_lib.ReplayRing()
        self._args = _keywalk_lib.Args()
        self._args.ring = ctypes.pointer(self._ring)
        self._args.n_step, self._args.gamma = self.n_step, self.gamma
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)      # what device_count=True reads

    _fill_ring = FusedReplaySampler._fill_ring          # the ring's addresses and sizes, checked: the same ring

    def push_count(self):
        """Copies mem.count into the device count (a fill launch, no host synchronisation): run it outside the graph
        before each replay of an extend captured with device_count=True."""
        self.count.fill_(self.mem.count)
        return self

    def _check(self, t, name, shape, dtypes):
        if not torch.is_tensor(t):
            raise TypeError(f"uavx: {name} must be a tensor, not {type(t).__name__}")
        if t.dtype not in dtypes or tuple(t.shape) != shape:
            raise ValueError(f"uavx: {name} must be {' or '.join(str(d) for d in dtypes)} {shape}, got {t.dtype} "
                             f"{tuple(t.shape)}")
        if t.device != self.device:
            raise ValueError(f"uavx: {name} is on {t.device}, the ring on {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"uavx: {name} must be contiguous")

    def extend(self, key, reward, next_state, mask, length=None, truncated=None, ended=None, device_count=False):
        """Overwrites reward [B], next_state [B, 10], mask [B] (float32) -- and truncated, ended (bool or uint8 [B], both or
        neither) and length (uint8 [B]) when given -- with the n-step values of the walks that start at key [B] int64;
        rows whose key is negative or outside the ring's window are left as they are, with length 0.  All tensors
        contiguous on the ring's device.  device_count=True: the kernel reads the ring's fill from the device count
        (push_count()).  Returns nothing it was not given: the tensors are written in place."""
        if not torch.is_tensor(key) or key.dtype != torch.int64 or key.dim() != 1:
            raise ValueError("uavx: key must be an int64 tensor of shape [rows]")
        rows = int(key.shape[0])
        if rows > _MAX_ROWS:
            raise ValueError(f"uavx: KeyWalk takes 0..{_MAX_ROWS} rows, got {rows}")
        f32, flag = (torch.float32,), (torch.bool, torch.uint8)
        self._check(key, "key", (rows,), (torch.int64,))
        self._check(reward, "reward", (rows,), f32)
        self._check(next_state, "next_state", (rows, _lib.OBS_DIM), f32)
        self._check(mask, "mask", (rows,), f32)
        if (truncated is None) != (ended is None):
            raise ValueError("uavx: truncated and ended go together: both or neither")
        if truncated is not None:
            self._check(truncated, "truncated", (rows,), flag)
            self._check(ended, "ended", (rows,), flag)
        if length is not None:
            self._check(length, "length", (rows,), (torch.uint8,))
        if self.mem.count < 1:
            raise ValueError("uavx: the replay memory is empty (count == 0): step it before sampling")
        self._fill_ring()
        self._launch(key, reward, next_state, mask, length, truncated, ended, device_count)

    def _launch(self, key, reward, next_state, mask, length, truncated, ended, device_count):
        """The launch on tensors that were checked; the ring's fields are filled."""
        rows = int(key.shape[0])
        if rows == 0:
            return
        a, dev = self._args, self.device
        a.count, a.count_dev = int(self.mem.count), self.count.data_ptr() if device_count else None
        a.key, a.rows = key.data_ptr(), rows
        a.reward, a.next_state, a.mask = reward.data_ptr(), next_state.data_ptr(), mask.data_ptr()
        a.length = None if length is None else length.data_ptr()
        a.truncated, a.ended = (None, None) if truncated is None else (truncated.data_ptr(), ended.data_ptr())
        with torch.cuda.device(dev):
            rc = self._lib.uavx_keywalk(ctypes.byref(a), stream(dev))
        _keywalk_lib.check(rc, "uavx_keywalk")


class PrioritizedNStepSampler(PrioritizedReplaySampler):
    _FLAGS_OUT, _LENGTH_OUT = (9, 10), (8, 10)          # the len(out) that ask for the flags / for the length

    def __init__(self, mem, alpha=0.6, beta=0.4, eps=1e-6, stratified=True, n_step=3, gamma=0.99):
        if not isinstance(mem, DeviceReplay):
            raise TypeError(f"uavx: PrioritizedNStepSampler takes a DeviceReplay, not {type(mem).__name__}")
        if mem.obs.device.type != "cuda":               # the ring's kind and place are looked at first
            raise ValueError(f"uavx: PrioritizedNStepSampler needs the ring on a GPU (cuda:N), it is on {mem.obs.device}: "
                             "there is no CPU path")
        check_walk(n_step, gamma, "PrioritizedNStepSampler")
        super().__init__(mem, alpha=alpha, beta=beta, eps=eps, stratified=stratified)
        self._walk = KeyWalk(mem, n_step, gamma)
        self.n_step, self.gamma = self._walk.n_step, self._walk.gamma
        # one ring description and one device count: the draw's _fill_state and push_count() serve the walk too
        self._walk._ring = self._ring
        self._walk._args.ring = ctypes.pointer(self._ring)
        self._walk.count = self.count

    def _begin(self, rows, with_flags, out, device_count, with_length=False):
        """Everything that can be refused before the uniforms are drawn -> (with_flags, outputs, length or None)."""
        length = None
        if out is not None:
            out = tuple(out)
            with_flags = with_flags or len(out) in self._FLAGS_OUT
            with_length = with_length or len(out) in self._LENGTH_OUT
            want = (9 if with_flags else 7) + int(with_length)
            if len(out) != want:
                raise ValueError(f"uavx: out must hold {want} tensors (state, action, reward, next_state, mask, weight, key"
                                 f"{', truncated, ended' if with_flags else ''}{', length' if with_length else ''}), got "
                                 f"{len(out)}")
            if with_length:
                length, out = out[-1], out[:-1]
                self._walk._check(length, "out[length]", (rows,), (torch.uint8,))
        with_flags, outs = super()._begin(rows, with_flags, out, device_count)
        if with_length and length is None:
            length = torch.empty((rows,), dtype=torch.uint8, device=self.device)
        return with_flags, outs, length

    def _extend(self, with_flags, outs, length, device_count):
        """The walk behind the draw, on the draw's own outputs -> what sample() returns."""
        tr, en = (outs[7], outs[8]) if with_flags else (None, None)
        self._walk._launch(outs[6], outs[2], outs[3], outs[4], length, tr, en, device_count)
        return tuple(outs) if length is None else tuple(outs) + (length,)

    def sample_from_uniforms(self, u, with_flags=False, out=None, device_count=False, with_length=False):
        """Refresh, the sample kernel and the walk on given uniforms u [B] float32, contiguous on the ring's device."""
        if not torch.is_tensor(u) or u.dtype != torch.float32 or u.dim() != 1:
            raise ValueError("uavx: the uniforms must be a float32 tensor of shape [rows]")
        if u.device != self.device:
            raise ValueError(f"uavx: the uniforms are on {u.device}, the ring on {self.device}")
        if not u.is_contiguous():
            raise ValueError("uavx: the uniforms must be contiguous")
        rows = self._rows(u.shape[0])
        with_flags, outs, length = self._begin(rows, with_flags, out, device_count, with_length)
        return self._extend(with_flags, self._launch(u, rows, with_flags, outs), length, device_count)

    def sample(self, batch_size, generator=None, with_flags=False, out=None, device_count=False, with_length=False):
        """(state, action, reward, next_state, mask, weight, key) of `batch_size` prioritized n-step rows: the parent's
        draw, with reward the discounted return of the len <= n_step steps walked from the drawn transition, next_state
        the observation len steps on and mask (1 - done_last) * gamma^(len - 1).  with_flags appends (truncated, ended)
        of the last row walked, with_length then len as uint8 (0 where key is -1).  out: 7 to 10 preallocated contiguous
        tensors (8: with the length, 9: with the flags, 10: both).  ONE torch.rand((rows,)), as the parent draws it: the
        generator advances alike.  A refused call leaves the generator where it was."""
        rows = self._rows(batch_size)
        with_flags, outs, length = self._begin(rows, with_flags, out, device_count, with_length)
        u = self._u.get(rows)
        if u is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"uavx: the uniforms of a {rows}-row batch must exist before a graph capture: call "
                                   f"reserve({rows}) or sample({rows}) once first")
            u = self.reserve(rows)._u[rows]
        torch.rand((rows,), generator=generator, out=u)
        return self._extend(with_flags, self._launch(u, rows, with_flags, outs), length, device_count)

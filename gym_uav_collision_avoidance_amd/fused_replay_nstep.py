"""NStepReplaySampler: n-step returns and recency-weighted draws from a DeviceReplay as one HIP launch (two above 1024
rows) behind the two torch.rand calls (libuavx_replayx.so, include/uavx_nstep.h).

    sampler = NStepReplaySampler(mem, n_step=3, gamma=0.99, recency=0.8)
    s, a, R, s_n, m = sampler.sample(256, generator=g)      # R = sum_{j<len} gamma^j r_j, s_n = the observation len steps on,
                                                            # m = (1 - done_last) * gamma^(len-1)
    ..., tr, en = sampler.sample(256, with_flags=True)      # the flags of the last row walked
    ..., length = sampler.sample(256, with_length=True)     # len per row, uint8 in 1..n_step (after the flags, if both)

It has the surface of FusedReplaySampler (sample, sample_from_uniforms, reserve, push_count, workspace_bytes, count), so a
learner holds either: the TD target y = r + (mask * gamma) * (...) of the unchanged launches becomes
R + gamma^len * (1 - done_last) * (...).  With recency == 0 the uniforms are drawn exactly as FusedReplaySampler.sample
draws them (two torch.rand((3, B))), so the generator advances alike and n_step = 1 reproduces mem.sample bit for bit;
otherwise two torch.rand((5, B)): rows 3 and 4 are the second step index and the per-row coin (u < recency: the start
row is the NEWER of the two indices, which weighs the m-th oldest step of the window by m + 1/2).
There is NO fallback: anything the kernels do not implement raises before a launch and before the generator moves."""
import ctypes
import operator

import torch

from . import _lib, _replayx_lib
from ._fused_common import stream
from .fused_replay import FusedReplaySampler
from .replay import DeviceReplay

_MAX_ROWS = _replayx_lib.NSTEP_MAX_ROWS
N_STEP_MAX = _replayx_lib.NSTEP_MAX


def check_n_step(n_step, recency, who="NStepReplaySampler"):
    """n_step in 1..8 and recency in [0, 1] as (int, float), refused otherwise."""
    try:
        n = operator.index(n_step)
    except TypeError:
        n = 0
    if not 1 <= n <= N_STEP_MAX:
        raise ValueError(f"uavx: {who} takes n_step in 1..{N_STEP_MAX}, got {n_step!r}")
    try:
        r = float(recency)
    except (TypeError, ValueError):
        r = float("nan")
    if not 0.0 <= r <= 1.0:
        raise ValueError(f"uavx: {who} takes recency in [0, 1], got {recency!r}")
    return n, r


class NStepReplaySampler(FusedReplaySampler):
    def __init__(self, mem, n_step=3, gamma=0.99, recency=0.0):
        if not isinstance(mem, DeviceReplay):
            raise TypeError(f"uavx: NStepReplaySampler takes a DeviceReplay, not {type(mem).__name__}")
        device = mem.obs.device
        if device.type != "cuda":
            raise ValueError(f"uavx: NStepReplaySampler needs the ring on a GPU (cuda:N), it is on {device}: there is "
                             "no CPU path")
        self.n_step, self.recency = check_n_step(n_step, recency)
        self.gamma = float(gamma)
        if not 0.0 < self.gamma <= 1.0:
            raise ValueError(f"uavx: NStepReplaySampler takes gamma in (0, 1], got {gamma!r}")
        super().__init__(mem)
        self._xlib = _replayx_lib.load()
        self._args = _replayx_lib.NStepArgs()
        self._args.ring = ctypes.pointer(self._ring)
        self._cols = 5 if self.recency > 0.0 else 3       # the rows of uniforms sample() draws per draw

    def workspace_bytes(self, rows):
        n = ctypes.c_int64()
        _replayx_lib.check(self._xlib.uavx_nstep_workspace_bytes(self._rows(rows), ctypes.byref(n)),
                           f"uavx_nstep_workspace_bytes({rows})")
        return n.value

    @staticmethod
    def _rows(rows):
        rows = int(rows)
        if not 0 <= rows <= _MAX_ROWS:
            raise ValueError(f"uavx: NStepReplaySampler takes 0..{_MAX_ROWS} rows, got {rows}")
        return rows

    def _outputs(self, rows, with_flags, out, with_length=False):
        dev = self.device
        shapes = [((rows, _lib.OBS_DIM), torch.float32), ((rows, 2), torch.float32), ((rows,), torch.float32),
                  ((rows, _lib.OBS_DIM), torch.float32), ((rows,), torch.float32)]
        names = ["state", "action", "reward", "next_state", "mask"]
        if with_flags:
            shapes += [((rows,), torch.bool)] * 2
            names += ["truncated", "ended"]
        if with_length:
            shapes += [((rows,), torch.uint8)]
            names += ["length"]
        if out is None:
            # the flags are 0 / 1 bytes written by the kernel, handed out as bool like DeviceReplay.sample's
            return tuple(torch.empty(s, dtype=torch.uint8, device=dev).view(torch.bool) if d is torch.bool
                         else torch.empty(s, dtype=d, device=dev) for s, d in shapes)
        if len(out) != len(shapes):
            raise ValueError(f"uavx: out must hold {len(shapes)} tensors ({', '.join(names)}), got {len(out)}")
        for t, name, (shape, dtype) in zip(out, names, shapes):
            if not torch.is_tensor(t):
                raise TypeError(f"uavx: out[{name}] must be a tensor, not {type(t).__name__}")
            if tuple(t.shape) != shape or t.dtype != dtype:
                raise ValueError(f"uavx: out[{name}] must be {dtype} {shape}, got {t.dtype} {tuple(t.shape)}")
            if t.device != dev:
                raise ValueError(f"uavx: out[{name}] is on {t.device}, the ring on {dev}")
            if not t.is_contiguous():
                raise ValueError(f"uavx: out[{name}] must be contiguous")
        return out

    def _begin(self, rows, with_flags, out, with_length=False):
        """Everything that can be refused before the uniforms are drawn -> (with_flags, with_length, outputs)."""
        if self.mem.count < 1:
            raise ValueError("uavx: the replay memory is empty (count == 0): step it before sampling")
        self._fill_ring()
        if out is not None:
            out = tuple(out)
            with_flags = with_flags or len(out) in (7, 8)
            with_length = with_length or len(out) in (6, 8)
        self._ws.ensure(self.workspace_bytes(rows), rows)
        return with_flags, with_length, self._outputs(rows, with_flags, out, with_length)

    def _launch(self, u, rows, with_flags, outs, device_count, with_length=False):
        if rows == 0:
            return outs
        a = self._args
        a.count, a.count_dev = int(self.mem.count), self.count.data_ptr() if device_count else None
        a.u, a.u_cols, a.rows = u.data_ptr(), int(u.shape[1]), rows
        a.n_step, a.gamma, a.recency = self.n_step, self.gamma, self.recency
        a.state, a.action, a.reward, a.next_state, a.mask = (t.data_ptr() for t in outs[:5])
        a.truncated, a.ended = (outs[5].data_ptr(), outs[6].data_ptr()) if with_flags else (None, None)
        a.length = outs[-1].data_ptr() if with_length else None
        need = self.workspace_bytes(rows)
        a.workspace, a.workspace_bytes = (self._ws.buf.data_ptr() if need else None), self._ws.buf.numel()
        with torch.cuda.device(self.device):
            rc = self._xlib.uavx_nstep_sample(ctypes.byref(a), stream(self.device))
        _replayx_lib.check(rc, "uavx_nstep_sample")
        return outs

    def sample_from_uniforms(self, u, with_flags=False, out=None, device_count=False, with_length=False):
        """The kernel alone on given uniforms u [2, 3, B] (recency == 0 only) or [2, 5, B] float32 (first draw, redraw; rows
        k, e, i and, of five, the second k and the recency coin), contiguous on the ring's device.  with_flags, out,
        device_count, with_length: as sample()."""
        if (not torch.is_tensor(u) or u.dtype != torch.float32 or u.dim() != 3 or u.shape[0] != 2
                or u.shape[1] not in (3, 5)):
            raise ValueError("uavx: the uniforms must be a float32 tensor of shape [2, 3, rows] or [2, 5, rows]")
        if u.shape[1] == 3 and self.recency > 0.0:
            raise ValueError(f"uavx: recency = {self.recency} needs uniforms of shape [2, 5, rows], got [2, 3, rows]")
        if u.device != self.device:
            raise ValueError(f"uavx: the uniforms are on {u.device}, the ring on {self.device}")
        if not u.is_contiguous():
            raise ValueError("uavx: the uniforms must be contiguous")
        rows = self._rows(u.shape[2])
        with_flags, with_length, outs = self._begin(rows, with_flags, out, with_length)
        return self._launch(u, rows, with_flags, outs, device_count, with_length)

    def sample(self, batch_size, generator=None, with_flags=False, out=None, device_count=False, with_length=False):
        """(state, action, reward, next_state, mask) of `batch_size` n-step rows (include/uavx_nstep.h): reward the
        discounted return of the len <= n_step steps walked, next_state the observation len steps on, mask
        (1 - done_last) * gamma^(len - 1).  with_flags appends (truncated, ended) of the last row walked as bool,
        with_length then len as uint8.  out: 5 to 8 preallocated contiguous tensors of the result's shapes and dtypes
        (6: with the length, 7: with the flags, 8: both).  device_count=True: the window is derived in the kernel from the
        device count (push_count()), for a captured graph that is replayed while the ring grows.  A refused call leaves the
        generator where it was."""
        rows = self._rows(batch_size)
        with_flags, with_length, outs = self._begin(rows, with_flags, out, with_length)
        u = self._u.get(rows)
        if u is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"uavx: the uniforms of a {rows}-row batch must exist before a graph capture: call "
                                   f"sample({rows}) once first")
            u = self._u[rows] = torch.empty((2, self._cols, rows), dtype=torch.float32, device=self.device)
        torch.rand((self._cols, rows), generator=generator, out=u[0])
        torch.rand((self._cols, rows), generator=generator, out=u[1])
        return self._launch(u, rows, with_flags, outs, device_count, with_length)

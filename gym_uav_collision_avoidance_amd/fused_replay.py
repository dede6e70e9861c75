"""FusedReplaySampler: DeviceReplay.sample as one HIP launch (two above 1024 rows) behind the two torch.rand calls
(libuavx_actor.so, include/uavx_replay.h) instead of torch's forty small kernels.

    sampler = FusedReplaySampler(mem)                                  # a DeviceReplay, packed flags or not
    s, a, r, s2, m = sampler.sample(256, generator=g)                  # == mem.sample(256, generator=g), bit for bit
    s, a, r, s2, m, tr, en = sampler.sample(256, generator=g, with_flags=True)
    sampler.sample(256, generator=g, out=bufs)                         # preallocated outputs (graph capture)
    sampler.sample_from_uniforms(u)                                    # u [2, 3, B] float32: the kernel alone
    sampler.reserve(rows)                                              # workspace of a large batch, before a capture
    sampler.push_count(); sampler.sample(..., device_count=True)       # a captured sample follows mem.count

The uniforms are drawn exactly as DeviceReplay.sample draws them (two torch.rand((3, B)) from the generator, first draw
then redraw), so the generator advances alike and the batch is the same.  The ring is read where `mem` keeps it when the
call is made; a captured graph keeps those addresses, and with device_count=True reads the step count from a device
int64 that push_count() refreshes (a launch, not a host synchronisation) before each replay.

This is the one sampler implementation: it launches uavx_nstep_sample (include/uavx_nstep.h, §22), here with n_step = 1,
gamma = 1, recency = 0 and three columns of uniforms, which is uavx_replay_sample bit for bit.  NStepReplaySampler
(fused_replay_nstep.py) sets the walk and opens the `with_length` output.
There is NO fallback: anything the kernels do not implement raises before a launch."""
import ctypes

import torch

from . import _actor_lib, _lib
from ._fused_common import Workspace, stream
from .replay import DeviceReplay

_MAX_ROWS = _actor_lib.NSTEP_MAX_ROWS


class FusedReplaySampler:
    _COLS = (3,)                            # the columns of uniforms per draw that sample_from_uniforms takes
    _FLAGS_OUT, _LENGTH_OUT = (7,), ()      # the len(out) that ask for the flags / for the length

    def __init__(self, mem):
        who = type(self).__name__
        if not isinstance(mem, DeviceReplay):
            raise TypeError(f"uavx: {who} takes a DeviceReplay, not {type(mem).__name__}")
        self.mem = mem
        self.device = mem.obs.device
        if self.device.type != "cuda":
            raise ValueError(f"uavx: {who} needs the ring on a GPU (cuda:N), it is on {self.device}: there is "
                             "no CPU path")
        self._lib = _actor_lib.load()
        self._ring = _actor_lib.ReplayRing()
        self._args = _actor_lib.NStepArgs()
        self._args.ring = ctypes.pointer(self._ring)
        self._walk(1, 1.0, 0.0)
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)    # what device_count=True samples from
        self._ws = Workspace(self.device)
        self._u = {}      # rows -> [2, cols, rows] uniforms of sample(), allocated once per batch size

    def _walk(self, n_step, gamma, recency):
        """What never changes for a sampler, filled once: one step that keeps its reward and mask as they are."""
        a = self._args
        a.n_step, a.gamma, a.recency = n_step, gamma, recency
        self._recency = recency
        self._cols = 5 if recency > 0.0 else 3            # the rows of uniforms sample() draws per draw

    def workspace_bytes(self, rows):
        n = ctypes.c_int64()
        _actor_lib.check(self._lib.uavx_nstep_workspace_bytes(self._rows(rows), ctypes.byref(n)),
                         f"uavx_nstep_workspace_bytes({rows})")
        return n.value

    def reserve(self, rows):
        """Grows the workspace to what `rows` rows need (a graph capture cannot allocate it)."""
        self._ws.reserve(self.workspace_bytes(rows))
        return self

    def push_count(self):
        """Copies mem.count into the device count (a fill launch, no host synchronisation): run it outside the graph
        before each replay of a sample captured with device_count=True."""
        self.count.fill_(self.mem.count)
        return self

    @classmethod
    def _rows(cls, rows):
        rows = int(rows)
        if not 0 <= rows <= _MAX_ROWS:
            raise ValueError(f"uavx: {cls.__name__} takes 0..{_MAX_ROWS} rows, got {rows}")
        return rows

    def _fill_ring(self):
        """The ring's addresses and sizes as `mem` holds them now, checked against what the kernels index."""
        mem, dev, r = self.mem, self.device, self._ring
        L, E, N = mem.L, mem.env.num_envs, mem.env.num_agents
        want = (("obs", (L, E, N, _lib.OBS_DIM), torch.float32), ("act", (L, E, N, 2), torch.float32),
                ("rew", (L, E, N), torch.float32), ("done", (L, E, N), torch.uint8))
        if not mem.packed:
            want += (("skip", (L, E), torch.uint8), ("trunc", (L, E), torch.uint8), ("ended", (L, E), torch.uint8))
        for name, shape, dtype in want:
            t = getattr(mem, name)
            if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
                raise ValueError(f"uavx: ring tensor {name!r} must be a contiguous {dtype} {shape} on {dev}, it is "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}")
            setattr(r, name, t.data_ptr())
        if mem.packed:
            r.skip = r.trunc = r.ended = None
        r.slots, r.envs, r.agents, r.learners = L, E, N, mem.num_learners

    def _outputs(self, rows, with_flags, with_length, out):
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

    def _begin(self, rows, with_flags, with_length, out):
        """Everything that can be refused before the uniforms are drawn -> (with_flags, with_length, outputs)."""
        if self.mem.count < 1:
            raise ValueError("uavx: the replay memory is empty (count == 0): step it before sampling")
        self._fill_ring()
        if out is not None:
            out = tuple(out)
            with_flags = with_flags or len(out) in self._FLAGS_OUT
            with_length = with_length or len(out) in self._LENGTH_OUT
        self._ws.ensure(self.workspace_bytes(rows), rows)
        return with_flags, with_length, self._outputs(rows, with_flags, with_length, out)

    def _launch(self, u, rows, with_flags, with_length, outs, device_count):
        if rows == 0:
            return outs
        a = self._args
        a.count, a.count_dev = int(self.mem.count), self.count.data_ptr() if device_count else None
        a.u, a.u_cols, a.rows = u.data_ptr(), int(u.shape[1]), rows
        a.state, a.action, a.reward = outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr()
        a.next_state, a.mask = outs[3].data_ptr(), outs[4].data_ptr()
        a.truncated, a.ended = (outs[5].data_ptr(), outs[6].data_ptr()) if with_flags else (None, None)
        a.length = outs[-1].data_ptr() if with_length else None
        need = self.workspace_bytes(rows)
        a.workspace, a.workspace_bytes = (self._ws.buf.data_ptr() if need else None), self._ws.buf.numel()
        with torch.cuda.device(self.device):
            rc = self._lib.uavx_nstep_sample(ctypes.byref(a), stream(self.device))
        _actor_lib.check(rc, "uavx_nstep_sample")
        return outs

    def _from_uniforms(self, u, with_flags, with_length, out, device_count):
        shapes = " or ".join(f"[2, {c}, rows]" for c in self._COLS)
        if (not torch.is_tensor(u) or u.dtype != torch.float32 or u.dim() != 3 or u.shape[0] != 2
                or u.shape[1] not in self._COLS):
            raise ValueError(f"uavx: the uniforms must be a float32 tensor of shape {shapes}")
        if u.shape[1] < self._cols:
            raise ValueError(f"uavx: recency = {self._recency} needs uniforms of shape [2, 5, rows], got [2, 3, rows]")
        if u.device != self.device:
            raise ValueError(f"uavx: the uniforms are on {u.device}, the ring on {self.device}")
        if not u.is_contiguous():
            raise ValueError("uavx: the uniforms must be contiguous")
        rows = self._rows(u.shape[2])
        with_flags, with_length, outs = self._begin(rows, with_flags, with_length, out)
        return self._launch(u, rows, with_flags, with_length, outs, device_count)

    def _sample(self, batch_size, generator, with_flags, with_length, out, device_count):
        rows = self._rows(batch_size)
        with_flags, with_length, outs = self._begin(rows, with_flags, with_length, out)
        u = self._u.get(rows)
        if u is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"uavx: the uniforms of a {rows}-row batch must exist before a graph capture: call "
                                   f"sample({rows}) once first")
            u = self._u[rows] = torch.empty((2, self._cols, rows), dtype=torch.float32, device=self.device)
        torch.rand((self._cols, rows), generator=generator, out=u[0])
        torch.rand((self._cols, rows), generator=generator, out=u[1])
        return self._launch(u, rows, with_flags, with_length, outs, device_count)

    def sample_from_uniforms(self, u, with_flags=False, out=None, device_count=False):
        """The kernel alone on given uniforms u [2, 3, B] float32 (first draw, redraw; rows k, e, i), contiguous on the
        ring's device.  with_flags, out, device_count: as sample()."""
        return self._from_uniforms(u, with_flags, False, out, device_count)

    def sample(self, batch_size, generator=None, with_flags=False, out=None, device_count=False):
        """DeviceReplay.sample(batch_size, generator, with_flags), bit for bit, in two torch.rand launches and one HIP
        launch (two above 1024 rows).  out: 5 (or, for the flags too, 7) preallocated contiguous tensors of the result's
        shapes and dtypes that receive it.  device_count=True: the window is derived in the kernel from the device count
        (push_count()) instead of mem.count as it is now -- for a captured graph that is replayed while the ring grows.
        A refused call leaves the generator where it was."""
        return self._sample(batch_size, generator, with_flags, False, out, device_count)

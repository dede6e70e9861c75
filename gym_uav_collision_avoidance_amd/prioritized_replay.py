"""PrioritizedReplaySampler: proportional prioritized experience replay (Schaul et al.) on a DeviceReplay, in HIP
(libuavx_prio.so, include/uavx_prio.h): a priority per transition, a draw with probability p / total, the
importance-sampling weights, and the feedback of TD errors into the ring.

    per = PrioritizedReplaySampler(mem, alpha=0.6, beta=0.4)           # a DeviceReplay, packed flags or not
    s, a, r, s2, m, w, key = per.sample(256, generator=g)              # one torch.rand, refresh (2 launches), sample (1)
    per.update_priorities(key, q, y)                                   # |q − y| -> priorities; q [towers, B] or [B]
    per.update_priorities(key, td_abs)                                 # or the |TD errors| themselves
    per.set_beta(0.7)                                                  # through a device slot: a captured graph follows
    per.sample_from_uniforms(u)                                        # u [B] float32: refresh and the kernel alone
    per.reserve(rows); per.push_count(); per.sample(..., device_count=True)      # as FusedReplaySampler, for a capture
    per.priorities, per.set_priorities(table)                          # the raw uint32 [slots, envs, learners] table
    per.state_dict(), per.load_state_dict(sd)                          # table, record, alpha, beta, eps

Priorities are integers, uint32 in Q16.16 (65 536 is 1.0, 0 cannot be drawn), and every sum over them is a uint64: the
drawn rows are a pure function of the table and the uniforms.  New transitions enter at the largest priority seen so far.
Rows where the env was re-initialised, rows DeviceReplay.reset took out and the ring's head have priority 0.  A batch is
one-step: (state, action, reward, next_state, mask) as DeviceReplay.sample gathers them, then weight [B] float32 --
(N·P)^−beta over its maximum -- and key [B] int64, which names the transition for update_priorities and goes stale (is
ignored) once the ring has overwritten it.  With nothing to draw (every row invalid) key is −1 and weight 0.
There is NO fallback: anything the kernels do not implement raises before a launch."""
import ctypes

import torch

from . import _lib, _prio_lib
from ._fused_common import capture_guard, check_f32, stream
from .fused_replay import FusedReplaySampler
from .replay import DeviceReplay

_MAX_ROWS = _prio_lib.MAX_ROWS


def check_prioritized(alpha, eps, who="PrioritizedReplaySampler"):
    """alpha in [0, 1] and eps > 0 as floats, or a ValueError in `who`'s name."""
    def number(x):
        try:
            return float(x)
        except (TypeError, ValueError):
            return float("nan")

    a, e = number(alpha), number(eps)
    if not 0.0 <= a <= 1.0:
        raise ValueError(f"uavx: {who} takes a priority exponent alpha in [0, 1], got {alpha}")
    if not (e > 0.0 and e != float("inf")):
        raise ValueError(f"uavx: {who} takes a finite eps > 0, got {eps}")
    return a, e


def _check_beta(beta):
    try:
        b = float(beta)
    except (TypeError, ValueError):
        b = float("nan")                 # refused below
    if not 0.0 <= b <= 1.0:
        raise ValueError(f"uavx: PrioritizedReplaySampler takes beta in [0, 1], got {beta}")
    return b


class PrioritizedReplaySampler:
    _FLAGS_OUT = (9,)

    def __init__(self, mem, alpha=0.6, beta=0.4, eps=1e-6, stratified=True):
        if not isinstance(mem, DeviceReplay):
            raise TypeError(f"uavx: PrioritizedReplaySampler takes a DeviceReplay, not {type(mem).__name__}")
        self.mem = mem
        self.device = mem.obs.device
        if self.device.type != "cuda":
            raise ValueError(f"uavx: PrioritizedReplaySampler needs the ring on a GPU (cuda:N), it is on {self.device}: "
                             "there is no CPU path")
        self.alpha, self.eps = check_prioritized(alpha, eps)
        self.stratified = bool(stratified)
        L, E, NL = mem.L, mem.env.num_envs, mem.num_learners
        self.entries = L * E * NL
        if self.entries > _prio_lib.MAX_ENTRIES:
            raise ValueError(f"uavx: PrioritizedReplaySampler holds at most 2^26 priorities (slots x envs x learners), this "
                             f"ring has {L} x {E} x {NL} = {self.entries}")
        self._lib = _prio_lib.load()
        n = ctypes.c_int64()
        _prio_lib.check(self._lib.uavx_prio_state_bytes(self.entries, ctypes.byref(n)), "uavx_prio_state_bytes")
        dev = self.device
        self._table = torch.zeros((L, E, NL), dtype=torch.int32, device=dev)       # the uint32 bits
        self._sums = torch.zeros(n.value, dtype=torch.uint8, device=dev)
        self._rec = torch.zeros(_prio_lib.RECORD_BYTES // 8, dtype=torch.int64, device=dev)
        self._rec.view(torch.int32)[3] = _prio_lib.ONE                              # p_max
        self.count = torch.zeros(1, dtype=torch.int64, device=dev)                  # what device_count=True reads
        self._beta = torch.zeros(1, dtype=torch.float32, device=dev)
        self.set_beta(beta)
        self._ring = _prio_lib.ReplayRing()
        self._state = _prio_lib.State()
        self._state.ring = ctypes.pointer(self._ring)
        self._args = _prio_lib.SampleArgs()
        self._u = {}          # rows -> [rows] uniforms of sample(), allocated once per batch size
        self._none = {}       # rows -> keys of −1: update_priorities' warm-up before a capture

    # ---- state ---------------------------------------------------------------------------------------------------------
    @property
    def priorities(self):
        """The raw table: uint32 [slots, envs, learners] in Q16.16 (a view, not a copy)."""
        return self._table.view(torch.uint32)

    def set_priorities(self, table):
        """Overwrites the table (uint32 or int32 bits, [slots, envs, learners]) and marks every step written so far as
        having its priority: the next refresh zeroes what cannot be drawn and changes nothing else."""
        t = torch.as_tensor(table)
        if t.dtype == torch.uint32:
            t = t.view(torch.int32)
        if t.dtype != torch.int32 or tuple(t.shape) != tuple(self._table.shape):
            raise ValueError(f"uavx: the priority table must be uint32 {tuple(self._table.shape)}, got {t.dtype} "
                             f"{tuple(t.shape)}")
        self._table.copy_(t)
        self._rec[2] = int(self.mem.count)
        return self

    def record(self):
        """The device record as a dict of Python ints (one device-to-host copy; it synchronises)."""
        r = self._rec.cpu()
        pm = r.view(torch.int32)[2:4].numpy().view("uint32")
        return {"total": int(r[0]), "p_min": int(pm[0]), "p_max": int(pm[1]), "seen": int(r[2]), "valid": int(r[3])}

    def set_beta(self, beta):
        """The importance-sampling exponent, host value and device slot (a fill launch, no synchronisation): a captured
        sample reads the slot, so an annealed beta needs no new capture."""
        self.beta = _check_beta(beta)
        self._beta.fill_(self.beta)
        return self

    def state_dict(self):
        return {"table": self._table.detach().cpu().clone(), "record": self._rec.detach().cpu().clone(),
                "alpha": self.alpha, "beta": self.beta, "eps": self.eps}

    def load_state_dict(self, sd):
        if tuple(sd["table"].shape) != tuple(self._table.shape):
            raise ValueError(f"uavx: the saved priority table is {tuple(sd['table'].shape)}, this ring's "
                             f"{tuple(self._table.shape)}")
        self.alpha, self.eps = check_prioritized(sd["alpha"], sd["eps"])
        self._table.copy_(sd["table"])
        self._rec.copy_(sd["record"])
        return self.set_beta(sd["beta"])

    def reserve(self, rows):
        """Allocates what a graph capture of `rows` rows cannot: the uniforms of sample()."""
        rows = self._rows(rows)
        if rows not in self._u:
            capture_guard("uniforms", rows)
            self._u[rows] = torch.empty((rows,), dtype=torch.float32, device=self.device)
            self._none[rows] = torch.full((rows,), -1, dtype=torch.int64, device=self.device)
        return self

    def push_count(self):
        """Copies mem.count into the device count (a fill launch, no host synchronisation): run it outside the graph
        before each replay of calls captured with device_count=True."""
        self.count.fill_(self.mem.count)
        return self

    @staticmethod
    def _rows(rows):
        rows = int(rows)
        if not 0 <= rows <= _MAX_ROWS:
            raise ValueError(f"uavx: PrioritizedReplaySampler takes 0..{_MAX_ROWS} rows, got {rows}")
        return rows

    _fill_ring = FusedReplaySampler._fill_ring          # the ring's addresses and sizes, checked: the same ring

    def _fill_state(self, device_count):
        if self.mem.count < 1:
            raise ValueError("uavx: the replay memory is empty (count == 0): step it before sampling")
        self._fill_ring()
        st = self._state
        st.count, st.count_dev = int(self.mem.count), self.count.data_ptr() if device_count else None
        st.table, st.sums, st.sums_bytes = self._table.data_ptr(), self._sums.data_ptr(), self._sums.numel()
        st.rec = self._rec.data_ptr()
        return st

    # ---- sampling ------------------------------------------------------------------------------------------------------
    def _outputs(self, rows, with_flags, out):
        dev = self.device
        shapes = [((rows, _lib.OBS_DIM), torch.float32), ((rows, 2), torch.float32), ((rows,), torch.float32),
                  ((rows, _lib.OBS_DIM), torch.float32), ((rows,), torch.float32), ((rows,), torch.float32),
                  ((rows,), torch.int64)]
        names = ["state", "action", "reward", "next_state", "mask", "weight", "key"]
        if with_flags:
            shapes += [((rows,), torch.bool)] * 2
            names += ["truncated", "ended"]
        if out is None:
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

    def _begin(self, rows, with_flags, out, device_count):
        """Everything that can be refused before the uniforms are drawn -> (with_flags, outputs)."""
        self._fill_state(device_count)
        if out is not None:
            out = tuple(out)
            with_flags = with_flags or len(out) in self._FLAGS_OUT
        return with_flags, self._outputs(rows, with_flags, out)

    def refresh(self, device_count=False):
        """uavx_prio_refresh alone (two launches): sample() runs it itself."""
        st = self._fill_state(device_count)
        with torch.cuda.device(self.device):
            rc = self._lib.uavx_prio_refresh(ctypes.byref(st), stream(self.device))
        _prio_lib.check(rc, "uavx_prio_refresh")
        return self

    def _launch(self, u, rows, with_flags, outs):
        if rows == 0:
            return outs
        st, a, dev = self._state, self._args, self.device
        a.u, a.rows, a.stratified = u.data_ptr(), rows, int(self.stratified)
        a.beta, a.beta_dev = self.beta, self._beta.data_ptr()
        a.state, a.action, a.reward = outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr()
        a.next_state, a.mask, a.weight, a.key = (outs[3].data_ptr(), outs[4].data_ptr(), outs[5].data_ptr(),
                                                 outs[6].data_ptr())
        a.truncated, a.ended = (outs[7].data_ptr(), outs[8].data_ptr()) if with_flags else (None, None)
        with torch.cuda.device(dev):
            rc = self._lib.uavx_prio_refresh(ctypes.byref(st), stream(dev))
            _prio_lib.check(rc, "uavx_prio_refresh")
            rc = self._lib.uavx_prio_sample(ctypes.byref(st), ctypes.byref(a), stream(dev))
        _prio_lib.check(rc, "uavx_prio_sample")
        return outs

    def sample_from_uniforms(self, u, with_flags=False, out=None, device_count=False):
        """Refresh and the sample kernel on given uniforms u [B] float32, contiguous on the ring's device."""
        if not torch.is_tensor(u) or u.dtype != torch.float32 or u.dim() != 1:
            raise ValueError("uavx: the uniforms must be a float32 tensor of shape [rows]")
        if u.device != self.device:
            raise ValueError(f"uavx: the uniforms are on {u.device}, the ring on {self.device}")
        if not u.is_contiguous():
            raise ValueError("uavx: the uniforms must be contiguous")
        rows = self._rows(u.shape[0])
        with_flags, outs = self._begin(rows, with_flags, out, device_count)
        return self._launch(u, rows, with_flags, outs)

    def sample(self, batch_size, generator=None, with_flags=False, out=None, device_count=False):
        """(state, action, reward, next_state, mask, weight, key), with_flags=True appending (truncated, ended): ONE
        torch.rand((rows,)), the refresh and the draw.  out: 7 (or, for the flags too, 9) preallocated contiguous tensors.
        device_count=True: the kernels read the ring's fill from the device count (push_count()).  A refused call leaves
        the generator where it was."""
        rows = self._rows(batch_size)
        with_flags, outs = self._begin(rows, with_flags, out, device_count)
        u = self._u.get(rows)
        if u is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"uavx: the uniforms of a {rows}-row batch must exist before a graph capture: call "
                                   f"reserve({rows}) or sample({rows}) once first")
            u = self.reserve(rows)._u[rows]
        torch.rand((rows,), generator=generator, out=u)
        return self._launch(u, rows, with_flags, outs)

    # ---- feedback ------------------------------------------------------------------------------------------------------
    def update_priorities(self, key, q, y=None, device_count=False):
        """TD errors back into the table (two launches).  key [B] int64 as sample() returned it; q [towers, B] (or [B])
        float32 and y [B] or [B, 1] float32: the priority comes from max over the towers of |q − y|; with y=None q holds
        the |TD errors| themselves.  Stale keys (overwritten since) and keys of −1 are ignored; a key that occurs several
        times ends at the largest of its priorities."""
        dev = self.device
        if not torch.is_tensor(key) or key.dtype != torch.int64 or key.dim() != 1 or key.device != dev:
            raise ValueError(f"uavx: key must be an int64 tensor of shape [rows] on {dev}")
        rows = self._rows(key.shape[0])
        check_f32(q, dev, "q")
        if q.dim() == 1:
            q = q.unsqueeze(0)
        if q.dim() != 2 or q.shape[1] != rows or not 1 <= q.shape[0] <= _prio_lib.MAX_TOWERS:
            raise ValueError(f"uavx: q must be [towers, {rows}] with 1..{_prio_lib.MAX_TOWERS} towers (or [{rows}]), got "
                             f"{tuple(q.shape)}")
        if not key.is_contiguous() or not q.is_contiguous():
            raise ValueError("uavx: key and q must be contiguous")
        towers, y_ptr, y_stride = int(q.shape[0]), None, 1
        if y is None:
            if towers != 1:
                raise ValueError("uavx: without y, q holds the |TD errors| themselves: one row, not one per tower")
        else:
            check_f32(y, dev, "y")
            if tuple(y.shape) not in ((rows,), (rows, 1)):
                raise ValueError(f"uavx: y must be [{rows}] or [{rows}, 1], got {tuple(y.shape)}")
            y_ptr, y_stride = y.data_ptr(), (y.stride(0) if rows > 1 else 1)
            if y_stride < 1:
                raise ValueError("uavx: y must have a positive row stride")
        st = self._fill_state(device_count)
        if rows == 0:
            return self
        with torch.cuda.device(dev):
            rc = self._lib.uavx_prio_update(ctypes.byref(st), key.data_ptr(), q.data_ptr(), towers, y_ptr, y_stride, rows,
                                            self.alpha, self.eps, stream(dev))
        _prio_lib.check(rc, "uavx_prio_update")
        return self

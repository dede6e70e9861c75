"""NStepReplaySampler: n-step returns and recency-weighted draws from a DeviceReplay as one HIP launch (two above 1024
rows) behind the two torch.rand calls (libuavx_actor.so, include/uavx_nstep.h).

    sampler = NStepReplaySampler(mem, n_step=3, gamma=0.99, recency=0.8)
    s, a, R, s_n, m = sampler.sample(256, generator=g)      # R = sum_{j<len} gamma^j r_j, s_n = the observation len steps on,
                                                            # m = (1 - done_last) * gamma^(len-1)
    ..., tr, en = sampler.sample(256, with_flags=True)      # the flags of the last row walked
    ..., length = sampler.sample(256, with_length=True)     # len per row, uint8 in 1..n_step (after the flags, if both)

It is FusedReplaySampler (fused_replay.py: one implementation, one launch path) with the walk set and the length output
opened, so a learner holds either: the TD target y = r + (mask * gamma) * (...) of the unchanged launches becomes
R + gamma^len * (1 - done_last) * (...).  With recency == 0 the uniforms are drawn exactly as FusedReplaySampler.sample
draws them (two torch.rand((3, B))), so the generator advances alike and n_step = 1 reproduces mem.sample bit for bit;
otherwise two torch.rand((5, B)): rows 3 and 4 are the second step index and the per-row coin (u < recency: the start
row is the NEWER of the two indices, which weighs the m-th oldest step of the window by m + 1/2).
There is NO fallback: anything the kernels do not implement raises before a launch and before the generator moves."""
import operator

from . import _actor_lib
from .fused_replay import FusedReplaySampler

N_STEP_MAX = _actor_lib.NSTEP_MAX


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
    _COLS = (3, 5)
    _FLAGS_OUT, _LENGTH_OUT = (7, 8), (6, 8)

    def __init__(self, mem, n_step=3, gamma=0.99, recency=0.0):
        super().__init__(mem)               # the ring's kind and place are looked at first
        self.n_step, self.recency = check_n_step(n_step, recency)
        self.gamma = float(gamma)
        if not 0.0 < self.gamma <= 1.0:
            raise ValueError(f"uavx: NStepReplaySampler takes gamma in (0, 1], got {gamma!r}")
        self._walk(self.n_step, self.gamma, self.recency)

    def sample_from_uniforms(self, u, with_flags=False, out=None, device_count=False, with_length=False):
        """The kernel alone on given uniforms u [2, 3, B] (recency == 0 only) or [2, 5, B] float32 (first draw, redraw; rows
        k, e, i and, of five, the second k and the recency coin), contiguous on the ring's device.  with_flags, out,
        device_count, with_length: as sample()."""
        return self._from_uniforms(u, with_flags, with_length, out, device_count)

    def sample(self, batch_size, generator=None, with_flags=False, out=None, device_count=False, with_length=False):
        """(state, action, reward, next_state, mask) of `batch_size` n-step rows (include/uavx_nstep.h): reward the
        discounted return of the len <= n_step steps walked, next_state the observation len steps on, mask
        (1 - done_last) * gamma^(len - 1).  with_flags appends (truncated, ended) of the last row walked as bool,
        with_length then len as uint8.  out: 5 to 8 preallocated contiguous tensors of the result's shapes and dtypes
        (6: with the length, 7: with the flags, 8: both).  device_count=True: the window is derived in the kernel from the
        device count (push_count()), for a captured graph that is replayed while the ring grows.  A refused call leaves the
        generator where it was."""
        return self._sample(batch_size, generator, with_flags, with_length, out, device_count)

"""Exploration: the collection side of the reference's trainers as one HIP launch behind the actor's forward
(libuavx_actor.so, include/uavx_explore.h).

    ex = agent.exploration(mem, seed=1, warmup_steps=64)          # or Exploration(fused_actor, rows, ...)
    agent.select_action(mem.state, explore=ex, out=mem.action_slot())
    mem.step(polar=True)

Per acting row it keeps 16 bytes on the device: the value of the row's Ornstein-Uhlenbeck process (ou.py) and the number of
calls the row has seen.  While that number is below `warmup_steps`, or with probability `random_prob` afterwards, the row
acts uniformly in [-1, 1] (np.random.uniform(-1, 1) of the trainers); otherwise SAC samples tanh(mean + std·n), TD3 adds
noise_std·n and clips, DDPG adds its OU value to both components and clips.  The normals are Philox4x32-10 draws keyed by
(seed, row_offset + row, call number): they depend on the GLOBAL row, not on how a batch is cut into shards, and nothing
is allocated per call.  act() is two launches, the RAW forward and the exploration kernel; both can be captured."""
import ctypes
import math

import torch

from . import _actor_lib
from ._fused_common import stream


def launch(lib, stream, **fields):
    """uavx_explore_act with the fields of uavx_explore_args (absent ones zero / NULL); returns the status."""
    args = _actor_lib.ExploreArgs()
    for k, v in fields.items():
        if not hasattr(args, k):
            raise TypeError(f"uavx: uavx_explore_args has no field {k!r}")
        setattr(args, k, v)
    return lib.uavx_explore_act(ctypes.byref(args), stream)


class Exploration:
    def __init__(self, actor, rows, seed=0, row_offset=0, warmup_steps=0, random_prob=0.0, noise_std=0.1, ou_sigma=0.2,
                 ou_theta=0.15, ou_dt=1e-2, ou_mean=0.0, ou_x_initial=0.0, reset_on_episode=False):
        """actor: a FusedActor (f32 or bf16) whose RAW forward feeds the launch.  rows: the acting rows of every call
        (num_envs * num_agents of a DeviceReplay).  seed, row_offset: the Philox key and the global row of row 0 (a shard
        passes its first global row).  warmup_steps: calls a row acts at random for; random_prob: the probability of a random
        action afterwards (set_random_prob anneals it).  noise_std: TD3's; ou_*: OUActionNoise's arguments (DDPG).
        reset_on_episode: restart a row's OU process at ou_x_initial when its env began a new episode (ddpg_tf2's trainer);
        the default never restarts it (pytorch_ddpg_temp's)."""
        from .fused_actor import FusedActor
        if not isinstance(actor, FusedActor):
            raise TypeError(f"uavx: Exploration takes a FusedActor, not {type(actor).__name__}")
        rows, seed, row_offset, warmup_steps = int(rows), int(seed), int(row_offset), int(warmup_steps)
        if not 1 <= rows <= _actor_lib.EXPLORE_MAX_ROWS:
            raise ValueError(f"uavx: Exploration needs 1 <= rows <= {_actor_lib.EXPLORE_MAX_ROWS}, got {rows}")
        if not 0 <= seed < 2 ** 64 or not 0 <= row_offset < 2 ** 63 or not 0 <= warmup_steps < 2 ** 63:
            raise ValueError("uavx: seed must be in [0, 2^64), row_offset and warmup_steps in [0, 2^63)")
        for name, v in (("noise_std", noise_std), ("ou_sigma", ou_sigma), ("ou_dt", ou_dt)):
            if not (math.isfinite(v) and v >= 0):
                raise ValueError(f"uavx: {name} must be finite and >= 0, got {v}")
        for name, v in (("ou_theta", ou_theta), ("ou_mean", ou_mean), ("ou_x_initial", ou_x_initial)):
            if not math.isfinite(v):
                raise ValueError(f"uavx: {name} must be finite, got {v}")
        self.actor, self.kind, self.device, self.rows = actor, actor.kind, actor.device, rows
        self.seed, self.row_offset, self.warmup_steps = seed, row_offset, warmup_steps
        self.noise_std, self.ou_sigma, self.ou_theta = float(noise_std), float(ou_sigma), float(ou_theta)
        self.ou_dt, self.ou_mean, self.ou_x_initial = float(ou_dt), float(ou_mean), float(ou_x_initial)
        self.reset_on_episode = bool(reset_on_episode)
        self.memory = None              # learners' exploration(memory) binds the ring act() reads the episode flags from
        self._lib = _actor_lib.load()
        self._cols = 4 if self.kind == _actor_lib.SAC else 2
        # one 16-byte row {double x; uint32 n; uint32 reserved} per acting row, seen as two float64 columns
        self.state = torch.zeros((rows, 2), dtype=torch.float64, device=self.device)
        self.state[:, 0] = self.ou_x_initial
        self._raw = torch.empty((rows, self._cols), dtype=torch.float32, device=self.device)
        self._prob = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.set_random_prob(random_prob)

    @property
    def ou_state(self):
        """The rows' OU values: a float64 [rows] view of the state."""
        return self.state[:, 0]

    @property
    def steps(self):
        """The rows' call counts: an int32 [rows] view of the state (the count wraps modulo 2^32; int32 shows it signed)."""
        return self.state.view(torch.int32)[:, 2]

    def set_random_prob(self, p):
        """The probability of a random action after the warm-up, written into the device slot the kernel reads with a
        stream-ordered fill: a captured act() follows it without a new capture."""
        p = float(p)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"uavx: random_prob must be in [0, 1], got {p}")
        self.random_prob = p
        self._prob.fill_(p)
        return self

    def state_dict(self):
        return {"state": self.state.detach().cpu().clone(), "random_prob": self.random_prob, "seed": self.seed,
                "row_offset": self.row_offset, "rows": self.rows}

    def load_state_dict(self, sd):
        if int(sd["rows"]) != self.rows or tuple(sd["state"].shape) != (self.rows, 2):
            raise ValueError(f"uavx: the saved exploration state has {sd['rows']} rows, this one {self.rows}")
        if int(sd["seed"]) != self.seed or int(sd["row_offset"]) != self.row_offset:
            raise ValueError("uavx: the saved exploration state was drawn with another seed or row_offset")
        self.state.copy_(sd["state"])
        return self.set_random_prob(sd["random_prob"])

    def _pair(self, t, what):
        if t is None:
            return None
        if (not torch.is_tensor(t) or t.dtype != torch.float64 or t.device != self.device
                or tuple(t.shape) != (self.rows, 2) or not t.is_contiguous()):
            raise ValueError(f"uavx: {what} must be a contiguous float64 [{self.rows}, 2] tensor on {self.device}")
        return t.data_ptr()

    def _flags(self, memory, reset):
        """(pointer, stride in bytes, mask, rows per env) of the reset flags, or None."""
        if reset is not None:
            if (not torch.is_tensor(reset) or reset.dtype != torch.uint8 or reset.device != self.device or reset.dim() != 1
                    or reset.shape[0] < 1 or self.rows % reset.shape[0]):
                raise ValueError(f"uavx: reset must be a uint8 [envs] tensor on {self.device} with envs dividing {self.rows}")
            return reset.data_ptr(), (reset.stride(0) if reset.shape[0] > 1 else 1), 1, self.rows // reset.shape[0]
        memory = self.memory if memory is None else memory
        if not self.reset_on_episode or memory is None or memory.count == 0:
            return None
        E, N = memory.env.num_envs, memory.env.num_agents
        if self.rows % E:
            raise ValueError(f"uavx: {self.rows} acting rows are no multiple of the memory's {E} envs")
        prev = (memory.count - 1) % memory.L
        if memory.packed:       # bit 1 ("re-initialised") of agent 0's done byte
            return memory.done[prev].data_ptr(), N, 2, self.rows // E
        return memory.skip[prev].data_ptr(), 1, 1, self.rows // E

    @torch.no_grad()
    def act(self, obs, out=None, memory=None, reset=None, normals=None, normals_out=None):
        """obs: float32 [..., 10] with `rows` rows in all.  out: a float32 [..., 2] tensor written in place and returned
        (e.g. DeviceReplay.action_slot()).  memory: with reset_on_episode, the DeviceReplay whose previous step's
        "re-initialised" flags restart the OU processes of the envs that began an episode; the slot is chosen on the host,
        so a graph of your own captures one slot.  reset: a uint8 [envs] tensor instead, non-zero bit 0 restarts.
        normals / normals_out: float64 [rows, 2]: feed the standard normals instead of drawing them / receive the pair used."""
        a = self.actor
        lead, o2 = a._rows(obs)
        if o2.shape[0] != self.rows:
            raise ValueError(f"uavx: this Exploration acts for {self.rows} rows, got {o2.shape[0]}")
        out = a._out(out, lead, 2)
        try:
            d2 = out.view(self.rows, 2)
        except RuntimeError:
            raise ValueError("uavx: out must be viewable as [rows, 2] with one row stride (written in place)") from None
        if d2.stride(1) != 1:
            raise ValueError("uavx: out must have unit stride along its last dimension")
        fields = dict(normals=self._pair(normals, "normals"), normals_out=self._pair(normals_out, "normals_out"))
        flags = self._flags(memory, reset)
        if flags is not None:
            fields.update(reset_flags=flags[0], reset_stride=flags[1], reset_mask=flags[2], rows_per_env=flags[3])
        a._launch(o2, None, 0.0, _actor_lib.RAW, self._raw, self._cols)
        rc = launch(self._lib, stream(self.device), kind=self.kind, rows=self.rows, row_offset=self.row_offset, seed=self.seed,
                    raw=self._raw.data_ptr(), raw_stride=self._cols, out=d2.data_ptr(),
                    out_stride=d2.stride(0) if self.rows > 1 else 2, state=self.state.data_ptr(),
                    warmup_steps=self.warmup_steps, random_prob_dev=self._prob.data_ptr(), random_prob=self.random_prob,
                    noise_std=self.noise_std, ou_sigma=self.ou_sigma, ou_theta=self.ou_theta, ou_dt=self.ou_dt,
                    ou_mean=self.ou_mean, ou_x_initial=self.ou_x_initial, **fields)
        _actor_lib.check(rc, "uavx_explore_act")
        return out

    __call__ = act

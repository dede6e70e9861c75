"""Crafted rings for the GAE(λ) tests (include/uavx_gae.h): values written straight into the ring tensors,
one layout per rule of the definition.  A layout is a function (E, N) -> case; a case is a dict of numpy arrays in the
UNPACKED flag layout plus count, steps, γ, λ and learners.  packed(case) moves the flags into bits 1 and 2 of agent 0's done
byte (and sets bit 3, "truncated", on some rows: the advantage pass must not look at it)."""
import numpy as np

T_SMALL = 5


def _base(E, N, T=T_SMALL, count=9, steps=None, gamma=0.99, lam=0.95, learners=None, seed=0, p_done=0.12, p_ended=0.1,
          p_skip=0.1):
    """A seeded ring of L = T + 1 slots with random rewards, values, dones, ended and skip rows."""
    rng = np.random.default_rng(1000 * seed + 17 * E + N)
    L = T + 1
    case = dict(T=T, E=E, N=N, count=count, steps=min(count, T) if steps is None else steps, gamma=gamma, lam=lam,
                learners=N if learners is None else learners,
                rew=rng.normal(size=(L, E, N)).astype(np.float32),
                values=rng.normal(size=(L, E, N)).astype(np.float32),
                done=(rng.random((L, E, N)) < p_done).astype(np.uint8),
                skip=(rng.random((L, E)) < p_skip).astype(np.uint8),
                ended=(rng.random((L, E)) < p_ended).astype(np.uint8))
    return case


def _slot(case, k):
    return k % (case["T"] + 1)


def _clean(E, N, **kw):
    """No dones, no flags: every column is one uncut walk."""
    return _base(E, N, p_done=0.0, p_ended=0.0, p_skip=0.0, **kw)


def _counts(count):
    return lambda E, N: _base(E, N, count=count, seed=count)


def _steps(steps):
    return lambda E, N: _base(E, N, count=9, steps=steps, seed=20 + steps)


def done_at_newest(E, N):
    c = _base(E, N, seed=31)
    c["done"][_slot(c, c["count"] - 1)] |= 1
    return c


def parked_agent(E, N):
    """Agent 0 of env 0 is done at k = 5 and stays parked (done = 1 in every later row) while its env goes on."""
    c = _clean(E, N, seed=32)
    for k in range(5, c["count"]):
        c["done"][_slot(c, k), 0, 0] = 1
    return c


def ended_with_and_without_done(E, N):
    """The env's episode ends at k = 6: agent 0 is done itself (no bootstrap), the others are not (they bootstrap)."""
    c = _clean(E, N, seed=33)
    c["ended"][_slot(c, 6), :] = 1
    c["done"][_slot(c, 6), :, 0] = 1
    return c


def two_adjacent_skips(E, N):
    c = _clean(E, N, seed=34)
    c["skip"][_slot(c, 5), 0] = 1
    c["skip"][_slot(c, 6), 0] = 1
    c["skip"][_slot(c, 6), E - 1] = 1
    return c


def skip_at_oldest_and_newest(E, N):
    c = _clean(E, N, seed=35)
    c["skip"][_slot(c, c["count"] - 1), 0] = 1
    c["skip"][_slot(c, c["count"] - c["steps"]), E - 1] = 1
    return c


def all_skip(E, N):
    c = _base(E, N, seed=36)
    c["skip"][:] = 1
    return c


def one_valid_entry(E, N):
    """Every row is a skip row but one, and one agent learns: n = 1."""
    c = _base(E, N, seed=37, learners=1)
    c["skip"][:] = 1
    c["skip"][_slot(c, 6), E - 1] = 0
    return c


def fewer_learners(E, N):
    return _base(E, N, seed=38, learners=max(1, N - 1))


def nan_not_bootstrapped(E, N):
    """NaN in the value of the newest successor state of a column whose agent is done there, and in the successors of the
    dones of a whole env in mid-window whose own row is a skip row: neither is read into an output."""
    c = _clean(E, N, seed=39)
    new = c["count"] - 1
    c["done"][_slot(c, new), 0, 0] = 1
    c["values"][_slot(c, new + 1), 0, 0] = np.nan
    c["done"][_slot(c, 5), E - 1, :] = 1
    c["skip"][_slot(c, 6), E - 1] = 1
    c["values"][_slot(c, 6), E - 1, :] = np.nan
    return c


def nan_bootstrapped(E, N):
    """NaN in the value the newest row of column (0, 0) bootstraps from: it runs down the column to the first stop."""
    c = _clean(E, N, seed=40)
    c["values"][_slot(c, c["count"]), 0, 0] = np.nan
    c["ended"][_slot(c, 6), 0] = 1
    return c


def negative_zero_rewards(E, N):
    c = _base(E, N, seed=41)
    c["rew"][:] = -0.0
    c["values"][:] = 0.0
    c["values"][::2] = -0.0
    return c


def _gamma_lambda(gamma, lam):
    return lambda E, N: _base(E, N, seed=50, gamma=gamma, lam=lam)


def large_mean(E, N):
    """|mean| / std of the advantages is about 1e4: γ = 0 and V = 0 make adv = r = 1e4 + N(0, 1)."""
    c = _clean(E, N, seed=60, gamma=0.0, lam=0.0)
    c["rew"] += np.float32(1e4)
    c["values"][:] = 0.0
    return c


LAYOUTS = {
    "count_3": _counts(3), "count_5": _counts(5), "count_9": _counts(9), "count_13": _counts(13),
    "steps_1": _steps(1), "steps_2": _steps(2), "steps_T": _steps(T_SMALL),
    "done_at_newest": done_at_newest, "parked_agent": parked_agent,
    "ended_with_and_without_done": ended_with_and_without_done,
    "two_adjacent_skips": two_adjacent_skips, "skip_at_oldest_and_newest": skip_at_oldest_and_newest,
    "all_skip": all_skip, "one_valid_entry": one_valid_entry, "fewer_learners": fewer_learners,
    "nan_not_bootstrapped": nan_not_bootstrapped, "nan_bootstrapped": nan_bootstrapped,
    "negative_zero_rewards": negative_zero_rewards,
    "gamma0_lambda0": _gamma_lambda(0.0, 0.0), "gamma0_lambda1": _gamma_lambda(0.0, 1.0),
    "gamma1_lambda0": _gamma_lambda(1.0, 0.0), "gamma1_lambda1": _gamma_lambda(1.0, 1.0),
    "gamma099_lambda095": _gamma_lambda(0.99, 0.95),
    "large_mean": large_mean,
}

DEFAULT_SHAPE = (3, 2)


def make(name, E=None, N=None):
    E, N = (DEFAULT_SHAPE[0] if E is None else E), (DEFAULT_SHAPE[1] if N is None else N)
    case = LAYOUTS[name](E, N)
    case["name"] = name
    return case


def big(E, N, T, learners=None, seed=70):
    """The seeded ring at a shape of the caller's: a wrapped window of T steps."""
    case = _base(E, N, T=T, count=2 * T + 3, learners=learners, seed=seed)
    case["name"] = f"big_{E}x{N}_T{T}"
    return case


def packed(case):
    """The same ring with the flags in agent 0's done byte: bit 1 skip, bit 2 ended; bit 3 (truncated) set on every third
    ended row.  Returns a new case whose skip and ended are None."""
    c = dict(case)
    done = case["done"].copy()
    done[:, :, 0] |= (case["skip"] != 0).astype(np.uint8) * 2
    done[:, :, 0] |= (case["ended"] != 0).astype(np.uint8) * 4
    trunc = (case["ended"] != 0) & ((np.arange(case["ended"].size).reshape(case["ended"].shape) % 3) == 0)
    done[:, :, 0] |= trunc.astype(np.uint8) * 8
    c["done"], c["skip"], c["ended"] = done, None, None
    return c


class CraftedRing:
    """What RolloutAdvantages and PPO read of a DeviceReplay, filled from a case (packed=True: from packed(case)): the ring
    tensors on `device`, count, T, L, num_learners, packed and an env with its shape.  No worlds behind it."""

    def __init__(self, case, device, packed_flags=False):
        import types

        import torch
        c = packed(case) if packed_flags else case
        self.T, self.L, self.count, self.num_learners, self.packed = c["T"], c["T"] + 1, c["count"], c["learners"], packed_flags
        self.env = types.SimpleNamespace(num_envs=c["E"], num_agents=c["N"], device=torch.device(device))
        shape = (self.L, c["E"], c["N"])
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.rew, self.done = put(c["rew"]), put(c["done"])
        zeros = np.zeros(shape[:2], np.uint8)
        self.skip = put(zeros if packed_flags else case["skip"])
        self.ended = put(zeros if packed_flags else case["ended"])
        self.trunc = put(zeros)
        self.obs = torch.zeros(shape + (10,), dtype=torch.float32, device=device)
        self.act = torch.zeros(shape + (2,), dtype=torch.float32, device=device)

    @property
    def state(self):
        return self.obs[self.count % self.L]

    def action_slot(self):
        return self.act[self.count % self.L]

    def _flags(self, s, e):
        if self.packed:
            b = self.done[s, e, 0]
            return (b & 2) != 0, (b & 8) != 0, (b & 4) != 0
        return self.skip[s, e] != 0, self.trunc[s, e] != 0, self.ended[s, e] != 0


def ref_args(case):
    """The arguments of gae_ref.gae / gae_loop."""
    return dict(rew=case["rew"], done=case["done"], values=case["values"], count=case["count"], steps=case["steps"],
                gamma=case["gamma"], lam=case["lam"], learners=case["learners"], skip=case["skip"], ended=case["ended"])

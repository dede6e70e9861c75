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


ROWS = 8                 # rows of a column the walk fetches together; the layout below plants its events around multiples of it
T_GROUPS = 3 * ROWS
GROUP_STEPS = (ROWS - 1, ROWS, ROWS + 1, 2 * ROWS - 1, 2 * ROWS, 2 * ROWS + 1, 3 * ROWS - 1, 3 * ROWS)


def row_groups(steps, wrapped, E=100, N=3, learners=2, seed=90):
    """A ring of T = 24 (L = 25) whose events are planted by walk position j (j = 0 is the newest row, step count − 1):
        env 0   skip at j = 7 (the last row of the first group of ROWS rows)
        env 1   skip at j = 8 (the first row of the second group)
        env 2   skip at j = 7 and at j = 8
        env 3   ended at j = 8
        env 4   agent 0 done at j = 15;  env 5: agent 1 done at j = 16
        env 6   agent 0 parked (done = 1) in the rows j = 16 ... 8, alive again from j = 7
        env 7   skip at j = 6 alone: the row at j = 8 is NOT cut (a cut taken from the wrong row of the first group would cut it;
                behind a skip row itself the carry is 0 and a cut changes no value)
    Envs 0-7 carry nothing else; every other env has dones, ended and skip rows at a rate of 3 %.  wrapped: count = 40, so
    the window wraps around the ring; otherwise count = steps and the window's oldest row is the ring's step 0 (an event
    whose j lies before step 0 is not planted)."""
    assert E >= 9 and N >= 2 and 1 <= steps <= T_GROUPS
    count = 40 if wrapped else steps
    c = _base(E, N, T=T_GROUPS, count=count, steps=steps, learners=learners, seed=seed, p_done=0.03, p_ended=0.03, p_skip=0.03)
    c["done"][:, :8], c["skip"][:, :8], c["ended"][:, :8] = 0, 0, 0
    planted = [("skip", ROWS - 2, 7, None), ("skip", ROWS - 1, 0, None), ("skip", ROWS, 1, None), ("skip", ROWS - 1, 2, None), ("skip", ROWS, 2, None),
               ("ended", ROWS, 3, None), ("done", 2 * ROWS - 1, 4, 0), ("done", 2 * ROWS, 5, 1)]
    planted += [("done", j, 6, 0) for j in range(ROWS, 2 * ROWS + 1)]
    for what, j, e, i in planted:
        k = count - 1 - j
        if k >= 0:
            c[what][(_slot(c, k), e) if i is None else (_slot(c, k), e, i)] = 1
    c["name"] = f"row_groups_s{steps}_{'wrapped' if wrapped else 'from0'}"
    return c


def ppo_ring(E=32, N=3, T=12, count=17, learners=2, seed=97):
    """The ring of the PPO update tests: 32 x 3, T = 12, two learners, count = 17 (a wrapped window of 12 steps = 768 rows),
    dones, ended and skip rows at 5 %, and planted in envs 0-2, which carry nothing else:
        env 0   agent 0 done at k = 8 and parked (done = 1) up to k = 13, its env going on
        env 1   agent 1 done at k = 9 and the env's episode ended in that row: its row at k = 10 is a sample again
        env 2   re-initialisation rows at k = 6 and k = 7, the done bit of agent 0 set in the row at k = 7 (no step, so it
                parks nobody: the row at k = 8 is a sample)"""
    c = _base(E, N, T=T, count=count, learners=learners, seed=seed, p_done=0.05, p_ended=0.05, p_skip=0.05)
    c["rew"] += np.float32(3)            # returns of one sign: an untrained value net's gradient norm is then above 1
    c["done"][:, :3], c["skip"][:, :3], c["ended"][:, :3] = 0, 0, 0
    for k in range(8, 14):
        c["done"][_slot(c, k), 0, 0] = 1
    c["done"][_slot(c, 9), 1, 1] = 1
    c["ended"][_slot(c, 9), 1] = 1
    c["skip"][_slot(c, 6), 2] = 1
    c["skip"][_slot(c, 7), 2] = 1
    c["done"][_slot(c, 7), 2, 0] = 1
    c["name"] = "ppo_ring"
    return c


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

"""Crafted rings for the running-statistics tests (include/uavx_norm.h): the rings of gae_layouts with an
observation tensor on top.  A case is a gae_layouts case plus obs [L, E, N, F] float32 from a seeded generator -- feature
OFFSET_FEATURE shifted by 1e4, so that its mean dwarfs its spread -- and first = count − steps, the fold's oldest step."""
import numpy as np

import gae_layouts
from gae_layouts import LAYOUTS, GROUP_STEPS, CraftedRing, packed  # noqa: F401

OFFSET_FEATURE = 3
F_DEFAULT = 10


def with_obs(case, F=F_DEFAULT, seed=5):
    c = dict(case)
    L, E, N = case["rew"].shape
    rng = np.random.default_rng(7000 + 31 * seed + 13 * E + N + F)
    obs = (rng.normal(size=(L, E, N, F)) * rng.uniform(0.1, 3.0, size=F)).astype(np.float32)
    obs[..., min(OFFSET_FEATURE, F - 1)] += np.float32(1e4)
    c["obs"], c["F"], c["first"] = obs, F, case["count"] - case["steps"]
    return c


def make(name, E=None, N=None, F=F_DEFAULT):
    return with_obs(gae_layouts.make(name, E, N), F)


def big(E, N, T, learners=None, seed=70, F=F_DEFAULT):
    return with_obs(gae_layouts.big(E, N, T, learners=learners, seed=seed), F)


def row_groups(steps, wrapped, F=F_DEFAULT):
    return with_obs(gae_layouts.row_groups(steps, wrapped), F)


def ppo_ring(F=F_DEFAULT):
    return with_obs(gae_layouts.ppo_ring(), F)


def thirds(case):
    """[(first, count)] of three successive folds that together cover the case's window (fewer when it is shorter)."""
    first, count = case["first"], case["count"]
    cuts = sorted({first, first + (count - first) // 3, first + 2 * (count - first) // 3, count})
    return list(zip(cuts[:-1], cuts[1:]))


def ring_args(case):
    """The ring arguments of the norm_ref folds."""
    return dict(done=case["done"], learners=case["learners"], skip=case["skip"], ended=case["ended"])


class Ring(CraftedRing):
    """A CraftedRing whose obs is the case's."""

    def __init__(self, case, device, packed_flags=False):
        import torch
        super().__init__(case, device, packed_flags)
        self.obs = torch.from_numpy(np.ascontiguousarray(case["obs"])).to(device)

"""Host-side checks of what PPO computes (ppo.py), no GPU needed: the float32 log density of the squashed
Gaussian against a float64 writing of its own out to |u| = 20, where the textbook form log(1 − tanh² + 1e-6) is off by five
orders of magnitude more than the bound; the parked mask against a per-element loop written from the docstring, on every
crafted ring in both flag layouts, with the window starting at the ring's step 0 and with the row before the window in the
slot the next step will overwrite; and the pieces of tests/ppo_ref.py that the GPU tests trust."""
import math

import numpy as np
import pytest
import torch

import gae_layouts
import ppo_ref


# ---- log π -------------------------------------------------------------------------------------------------------------------

def _log_prob_inputs():
    g = torch.Generator().manual_seed(2024)
    rows = 4096
    u = (torch.rand((rows, 2), generator=g, dtype=torch.float64) * 40.0 - 20.0).to(torch.float32)
    mean = torch.randn((rows, 2), generator=g, dtype=torch.float64).to(torch.float32)
    log_std = (torch.rand((rows, 2), generator=g, dtype=torch.float64) * 6.0 - 4.0).to(torch.float32)
    return mean, log_std, u


def test_log_prob_against_float64_out_to_saturation():
    """Tolerance 2^-19 · Σ|terms|: about ten float32 operations per action dimension, each within 2 ulp (2^-23 relative) of a
    quantity bounded by the sum of the terms' absolute values: 10 · 2 · 2^-24 < 2^-19."""
    from gym_uav_collision_avoidance_amd.ppo import log_prob
    mean, log_std, u = _log_prob_inputs()
    assert float(u.abs().max()) > 19.9 and float(log_std.min()) < -3.9 and float(log_std.max()) > 1.9
    want, scale = ppo_ref.log_density(mean.double(), log_std.double(), u.double())
    tol = 2.0 ** -19 * scale
    got = log_prob(mean, log_std, u)
    assert got.dtype == torch.float32 and got.shape == (4096,)
    err = (got.double() - want).abs()
    print(f"log_prob: worst |float32 - float64| / tolerance = {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())
    # the usual form saturates: 1 − tanh² is 0 in float32 from |u| ≈ 9 on, and the 1e-6 caps the correction at log 1e-6
    z = (u - mean) * torch.exp(-log_std)
    naive = (-0.5 * z * z - log_std - 0.5 * math.log(2.0 * math.pi) - torch.log(1.0 - torch.tanh(u) ** 2 + 1e-6)).sum(-1)
    miss = float(((naive.double() - want).abs() / tol).max())
    print(f"log(1 - tanh^2 + 1e-6): worst / tolerance = {miss:.3g}")
    assert miss > 1e5


def test_log_density_terms_are_the_textbook_density():
    """ppo_ref's own writing against scipy-free first principles at moderate u, where log(1 − tanh²) is harmless in float64."""
    g = torch.Generator().manual_seed(5)
    u = torch.rand((500, 2), generator=g, dtype=torch.float64) * 6.0 - 3.0
    mean, log_std = torch.randn((500, 2), generator=g, dtype=torch.float64), torch.rand((500, 2), generator=g, dtype=torch.float64) - 0.5
    got, scale = ppo_ref.log_density(mean, log_std, u)
    normal = torch.distributions.Normal(mean, log_std.exp())
    want = (normal.log_prob(u) - torch.log(1.0 - torch.tanh(u) ** 2)).sum(-1)
    assert bool(((got - want).abs() <= 1e-12 * scale).all()) and bool((scale >= got.abs()).all())


# ---- the parked mask -----------------------------------------------------------------------------------------------------------

def _parked_loop(case, steps):
    """From the docstring: the agent was already done before the step of that row -- the previous row's done, unless that row
    ended the episode or was a re-initialisation; nothing is parked before step 0.  (parked, kept by ended, kept by skip)"""
    L, E, nl, count = case["T"] + 1, case["E"], case["learners"], case["count"]
    out = np.zeros((3, steps, E, nl), bool)
    for n in range(steps):
        k = count - steps + n
        if k == 0:
            continue
        p = (k - 1) % L
        for e in range(E):
            for i in range(nl):
                if case["done"][p, e, i] & 1:
                    which = 1 if case["ended"][p, e] else 2 if case["skip"][p, e] else 0
                    out[which, n, e, i] = True
    return out


def _slot_before_the_window():
    """The row before the oldest row of a full window lies in slot count mod L, the slot the next step writes: a done there."""
    c = gae_layouts._clean(4, 3, seed=98)
    assert c["steps"] == c["T"] == 5 and (c["count"] - c["steps"] - 1) % (c["T"] + 1) == c["count"] % (c["T"] + 1)
    c["done"][c["count"] % (c["T"] + 1), 1, 0] = 1
    c["name"] = "slot_before_the_window"
    return c


def _parked_cases():
    cases = [gae_layouts.make(name, 4, 3) for name in sorted(gae_layouts.LAYOUTS)]
    cases += [gae_layouts.row_groups(24, True), gae_layouts.row_groups(9, False), gae_layouts.ppo_ring(), _slot_before_the_window()]
    return cases


@pytest.mark.parametrize("packed_flags", [False, True], ids=["rows", "packed"])
def test_parked_mask_against_a_loop_over_every_crafted_ring(packed_flags):
    from gym_uav_collision_avoidance_amd.ppo import PPO
    seen = np.zeros(3, np.int64)
    from_step_0 = 0
    for case in _parked_cases():
        steps = case["steps"]
        mem = gae_layouts.CraftedRing(case, "cpu", packed_flags)
        ppo = PPO(mem, minibatches=1, rollout=steps)
        got = ppo._parked(ppo.advantages.window(steps), mem.count - steps)
        want = _parked_loop(case, steps)
        assert got.dtype == torch.bool and tuple(got.shape) == want[0].shape, case["name"]
        assert np.array_equal(got.numpy(), want[0]), case["name"]
        seen += want.reshape(3, -1).sum(1)
        if case["count"] == steps:
            from_step_0 += 1
            assert not want[0][0].any()
        if case["name"] == "slot_before_the_window":
            assert want[0][0, 1, 0] and want[0].sum() == 1
    print("parked rows", seen[0], "kept by ended", seen[1], "kept by skip", seen[2], "windows from step 0:", from_step_0)
    assert seen.min() > 0 and from_step_0 >= 3


def test_weight_loop_is_valid_and_not_parked():
    """ppo_ref.weight_loop, which the GPU tests compare PPO's weight with, against the parked loop above and gae_ref's valid."""
    import gae_ref
    kinds = set()
    for case in _parked_cases():
        for c in (case, gae_layouts.packed(case)):
            w, why = ppo_ref.weight_loop(c["done"], c["skip"], c["ended"], c["count"], c["steps"], c["learners"])
            _, _, valid = gae_ref.gae(**gae_layouts.ref_args(c))
            slots = [k % (c["T"] + 1) for k in range(c["count"] - c["steps"], c["count"])]
            parked = _parked_loop(case, case["steps"])[0]
            assert np.array_equal(w, ((valid[slots][:, :, :c["learners"]] == 1) & ~parked).astype(np.float32)), case["name"]
            assert np.array_equal(w == 1, (why == 1) | (why == 4) | (why == 5))
            kinds |= set(np.unique(why).tolist())
    assert kinds == {1, 2, 3, 4, 5}


def test_ppo_ring_holds_what_its_docstring_says():
    c = gae_layouts.ppo_ring()
    assert (c["E"], c["N"], c["T"], c["count"], c["steps"], c["learners"]) == (32, 3, 12, 17, 12, 2)
    w, why = ppo_ref.weight_loop(c["done"], c["skip"], c["ended"], c["count"], c["steps"], c["learners"])
    row = lambda k: k - (c["count"] - c["steps"])
    assert w.size == 768
    assert [int(why[row(k), 0, 0]) for k in range(7, 16)] == [1, 1, 3, 3, 3, 3, 3, 3, 1] and (why[:, 0, 1] == 1).all()
    assert why[row(10), 1, 1] == 4 and why[row(9), 1, 1] == 1
    assert (why[row(6), 2] == 2).all() and (why[row(7), 2] == 2).all() and why[row(8), 2, 0] == 5 and why[row(8), 2, 1] == 1
    assert (why[:, 3:] == 2).any() and (why[:, 3:] == 3).any()                # and the low-rate rest has both kinds of zero

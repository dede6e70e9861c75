"""RolloutAdvantages (libuavx_gae.so, include/uavx_gae.h) on the MI355X: adv, ret, valid, adv_norm and the
stats record bit-identical to tests/gae_ref.py -- on every crafted layout in both flag layouts, at shapes of one partly filled
wavefront, several wavefronts with a ragged last workgroup and several workgroups, and on a ring written by real env steps
with resets, truncations and the wrap; rows outside the window untouched; two calls the same bytes; a call on a side stream.
Further: windows of 7, 8, 9, 15, 16, 17, 23 and 24 steps on a ring of T = 24 with events planted on the rows either side of
the walk's groups of eight rows, wrapped and from the ring's step 0; 1, 3, 5 and 7 agents per env at 280-300 columns, so that
an env's columns lie in two wavefronts and in two workgroups; 257 and 513 workgroups, where the last sum adds two and three
partials per thread.  A NaN matches any NaN (the header leaves its payload open)."""
import numpy as np
import pytest
import torch

import gae_layouts
import gae_ref
from gae_ref import same

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = 7


def _compute(mem, values, gamma, lam, steps, normalize=True, prefill=SENTINEL):
    from gym_uav_collision_avoidance_amd.rollout import RolloutAdvantages
    ra = RolloutAdvantages(mem, gamma=gamma, lam=lam, normalize=normalize)
    for t in ra.outputs:
        if t is not None:
            t.fill_(prefill)
    out = ra.compute(values, steps)
    return ra, out


def _check(ra, out, kw, normalize=True):
    """Every output against gae_ref, rows outside the window against the sentinel they were filled with."""
    adv, ret, valid = gae_ref.gae(fill=SENTINEL, **kw)
    got = [t.cpu().numpy() if t is not None else None for t in out]
    assert same(got[0], adv), "adv"
    assert same(got[1], ret), "ret"
    assert same(got[2], valid), "valid"
    if not normalize:
        assert got[3] is None
        return
    norm, (n, mean, std) = gae_ref.normalise(adv, valid, kw["count"], kw["steps"], fill=SENTINEL)
    assert same(got[3], norm), "adv_norm"
    assert int(ra.stats.n) == n
    assert same(np.float64([float(ra.stats.mean), float(ra.stats.std)]), np.float64([mean, std])), (ra.stats, mean, std)


def _run_case(case, packed_flags, normalize=True):
    mem = gae_layouts.CraftedRing(case, DEV, packed_flags)
    values = torch.from_numpy(case["values"]).to(DEV)
    ra, out = _compute(mem, values, case["gamma"], case["lam"], case["steps"], normalize)
    kw = gae_layouts.ref_args(gae_layouts.packed(case) if packed_flags else case)
    _check(ra, out, kw, normalize)
    return ra, out


@pytest.mark.parametrize("packed_flags", [False, True], ids=["rows", "packed"])
@pytest.mark.parametrize("name", sorted(gae_layouts.LAYOUTS))
def test_every_layout_equals_the_reference_bit_for_bit(name, packed_flags):
    _run_case(gae_layouts.make(name), packed_flags)


@pytest.mark.parametrize("shape", [(2, 3), (1, 2)], ids=["2x3", "1x2"])
@pytest.mark.parametrize("name", sorted(gae_layouts.LAYOUTS))
def test_every_layout_at_the_other_small_shapes(name, shape):
    _run_case(gae_layouts.make(name, *shape), packed_flags=name < "g")      # about half the layouts in each flag layout


@pytest.mark.parametrize("packed_flags", [False, True], ids=["rows", "packed"])
@pytest.mark.parametrize("shape", [(70, 4, 8, 3), (1024, 4, 32, None), (1024, 4, 32, 2)], ids=["70x4_l3", "1024x4_T32", "1024x4_l2"])
def test_several_wavefronts_and_workgroups(shape, packed_flags):
    E, N, T, learners = shape
    _run_case(gae_layouts.big(E, N, T, learners=learners), packed_flags)


@pytest.mark.parametrize("packed_flags", [False, True], ids=["rows", "packed"])
@pytest.mark.parametrize("wrapped", [True, False], ids=["count40", "count_steps"])
@pytest.mark.parametrize("steps", gae_layouts.GROUP_STEPS)
def test_windows_around_the_row_groups(steps, wrapped, packed_flags):
    """100 x 3, two learners, T = 24: windows of 7 ... 24 steps -- a full group of fetched rows followed by a ragged one, two
    and three groups -- with a skip, an ended, a done and a parked agent on the rows either side of a group boundary."""
    case = gae_layouts.row_groups(steps, wrapped)
    assert case["steps"] == steps and case["count"] == (40 if wrapped else steps)
    assert (case["E"], case["N"], case["learners"], case["T"]) == (100, 3, 2, 24)
    _run_case(case, packed_flags)


def _straddles(E, N, width):
    """Envs whose N columns e·N ... e·N + N − 1 lie in two different runs of `width` columns."""
    return [e for e in range(E) if (e * N) // width != (e * N + N - 1) // width]


@pytest.mark.parametrize("packed_flags", [False, True], ids=["rows", "packed"])
@pytest.mark.parametrize("shape", [(300, 1, None), (100, 3, None), (60, 5, 3), (40, 7, 1)], ids=["300x1", "100x3", "60x5_l3", "40x7_l1"])
def test_envs_across_wavefront_and_workgroup_edges(shape, packed_flags):
    """Agent counts that do not divide 64: an env's columns lie in two wavefronts, and in two workgroups, so col / agents,
    col % agents and the packed-flag read from agent 0's byte cross both edges.  300 x 1 is agents = 1."""
    E, N, learners = shape
    assert E * N > gae_ref.BLOCK
    if N > 1:
        assert _straddles(E, N, gae_ref.WAVE) and _straddles(E, N, gae_ref.BLOCK), (E, N)
    case = gae_layouts.big(E, N, 12, learners=learners, seed=73)
    assert case["count"] > case["T"] + 1 and case["steps"] == 12              # the window wraps
    _run_case(case, packed_flags)


@pytest.mark.parametrize("shape", [(16385, 4, 2, 257, 4, False), (43691, 3, 3, 513, 1, True)], ids=["257_workgroups", "513_workgroups"])
def test_more_workgroups_than_one_workgroup_has_threads(shape):
    """total() adds two and three partials per thread; the last workgroup holds 4 columns and 1 column."""
    E, N, T, blocks, last, packed_flags = shape
    assert -(-E * N // gae_ref.BLOCK) == blocks and E * N - (blocks - 1) * gae_ref.BLOCK == last
    ra, out = _run_case(gae_layouts.big(E, N, T, seed=74), packed_flags)
    assert int(ra.stats.n) > 256 * gae_ref.BLOCK


def test_without_normalisation_the_walk_alone_runs():
    ra, out = _run_case(gae_layouts.big(70, 4, 8, learners=3), False, normalize=False)
    assert int(ra.stats.n) == 0 and float(ra.stats.std) == 0.0              # the record is not touched


@pytest.mark.parametrize("packed_flags", [False, True], ids=["rows", "packed"])
def test_live_ring_with_resets_truncations_and_the_wrap(packed_flags):
    """64 envs x 2 agents, step_cap = 3, auto_reset = "agent0_done", 20 steps into a ring of T = 8: what the step launch
    itself wrote is read back and handed to the reference."""
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    E, N, T = 64, 2, 8
    env = BatchedMultiUAVWorld2D(E, num_agents=N, device=DEV, seed=11)
    mem = DeviceReplay(env, horizon=T, packed_flags=packed_flags)
    mem.begin(env.reset())
    g = torch.Generator(device=DEV).manual_seed(12)
    for _ in range(20):
        mem.action_slot().copy_(torch.rand((E, N, 2), generator=g, device=DEV) * 2 - 1)
        mem.step(polar=True, auto_reset="agent0_done", step_cap=3)
    values = torch.randn((T + 1, E, N), generator=g, device=DEV)
    sk, tr, en = mem._flags(slice(None), slice(None))
    seen = [int(sk.sum()), int(tr.sum()), int(en.sum())]
    assert min(seen) > 0, seen                                               # resets, truncations and episode ends are in it
    for steps in (T, 3):
        ra, out = _compute(mem, values, 0.99, 0.95, steps)
        kw = dict(rew=mem.rew.cpu().numpy(), done=mem.done.cpu().numpy(), values=values.cpu().numpy(), count=mem.count,
                  steps=steps, gamma=0.99, lam=0.95, learners=N,
                  skip=None if packed_flags else mem.skip.cpu().numpy(), ended=None if packed_flags else mem.ended.cpu().numpy())
        _check(ra, out, kw)
        assert 0 < int(ra.stats.n) < steps * E * N
    env.close()


def test_two_calls_give_identical_bytes_and_a_later_window_leaves_the_rest():
    case = gae_layouts.big(300, 4, 16, seed=71)
    mem = gae_layouts.CraftedRing(case, DEV)
    values = torch.from_numpy(case["values"]).to(DEV)
    ra, out = _compute(mem, values, 0.99, 0.95, case["steps"])
    first = [t.clone() for t in out] + [ra._record.clone()]
    out = ra.compute(values, case["steps"])
    for a, b in zip(first, list(out) + [ra._record]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # a shorter window afterwards rewrites its own rows only: the older rows keep the first call's bytes
    out = ra.compute(values, 2)
    kept = ra.window(case["steps"])[:-2]
    for a, b in zip(first[:4], out):
        assert torch.equal(a[kept].view(torch.uint8), b[kept].view(torch.uint8))


def test_call_on_a_side_stream():
    case = gae_layouts.big(70, 4, 8, learners=3, seed=72)
    mem = gae_layouts.CraftedRing(case, DEV)
    values = torch.from_numpy(case["values"]).to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        ra, out = _compute(mem, values, case["gamma"], case["lam"], case["steps"])
    side.synchronize()
    _check(ra, out, gae_layouts.ref_args(case))

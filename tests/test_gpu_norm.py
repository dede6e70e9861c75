"""RolloutNormalizer (libuavx_norm.so, include/uavx_norm.h) on the MI355X: the record after a fold, the carry,
obs_ring() and rewards() bit-identical to tests/norm_ref.py -- on every crafted layout in both flag layouts; across wavefront
and workgroup edges; on the row-group windows, wrapped and from the ring's step 0; with more partials than a workgroup has
threads; with 10 and with 7 features; over three successive folds whose episodes span the fold boundaries; a batch without a
sample leaves the record's bytes alone; a NaN is where the reference has it and nowhere else; out may be in; unaligned and
ragged element-wise calls; a side stream; two runs the same bytes; and a ring written by real env steps with resets.  A NaN
matches any NaN (the header leaves its payload open)."""
import numpy as np
import pytest
import torch

import norm_layouts
import norm_ref
from gae_ref import same

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _normalizer(mem, gamma, **kw):
    from gym_uav_collision_avoidance_amd.normalize import RolloutNormalizer
    return RolloutNormalizer(mem, gamma=gamma, **kw)


def _words(norm):
    return norm._record.cpu().numpy().view(np.uint64)


def _fold_and_check(case, packed_flags, windows=None, clip_obs=10.0, clip_reward=10.0):
    """Folds `windows` (default: the case's one window) on the GPU and in norm_ref; record and carry are compared after every
    fold, obs_ring() and rewards() at the end.  Returns (normalizer, reference record, reference carry)."""
    mem = norm_layouts.Ring(case, DEV, packed_flags)
    c = norm_layouts.packed(case) if packed_flags else case
    ra = norm_layouts.ring_args(c)
    windows = [(case["first"], case["count"])] if windows is None else windows
    mem.count = windows[0][0]
    norm = _normalizer(mem, case["gamma"], clip_obs=clip_obs, clip_reward=clip_reward)
    norm.folded_obs = norm.folded_ret = windows[0][0]
    rec, C = norm_ref.new_record(case["F"]), np.zeros((case["E"], case["N"]))
    for first, count in windows:
        mem.count = count
        norm.fold_returns()
        norm.fold_obs()
        assert norm.folded_obs == norm.folded_ret == count
        rec = norm_ref.fold_obs(rec, c["obs"], first=first, count=count, **ra)
        rec, C = norm_ref.fold_returns(rec, C, c["rew"], first=first, count=count, gamma=case["gamma"], **ra)
        assert norm_ref.same_words(_words(norm), norm_ref.words(rec)), ("record", first, count)
        assert same(norm.carry.cpu().numpy(), C), ("carry", first, count)
    assert same(norm.obs_ring().cpu().numpy(), norm_ref.apply_obs(rec, c["obs"], 1e-8, clip_obs)), "obs_ring"
    assert same(norm.rewards().cpu().numpy(), norm_ref.scale_rewards(rec, c["rew"], 1e-8, clip_reward)), "rewards"
    st = norm.stats
    mean, var, var_ret = norm_ref.variances(rec)
    assert int(st.n_obs) == rec["n_obs"] and int(st.n_ret) == rec["n_ret"]
    assert same(st.mean.cpu().numpy(), mean) and same(st.var.cpu().numpy(), var)
    assert same(np.float64(float(st.var_ret)), np.float64(var_ret))
    return norm, rec, C


@pytest.mark.parametrize("packed_flags", [False, True], ids=["rows", "packed"])
@pytest.mark.parametrize("name", sorted(norm_layouts.LAYOUTS))
def test_every_layout_equals_the_reference_bit_for_bit(name, packed_flags):
    case = norm_layouts.make(name)
    assert (case["E"], case["N"]) == (3, 2)
    _fold_and_check(case, packed_flags)


@pytest.mark.parametrize("packed_flags", [False, True], ids=["rows", "packed"])
@pytest.mark.parametrize("shape", [(130, 2, None), (100, 3, 2), (60, 5, 3)], ids=["130x2", "100x3_l2", "60x5_l3"])
def test_across_wavefront_and_workgroup_edges_in_three_folds(shape, packed_flags):
    """260 and 300 columns: two workgroups, the second ragged; 3 and 5 agents per env put an env's columns into two wavefronts
    and two workgroups.  Three successive folds: the carry and the parked look-back cross the fold boundaries."""
    E, N, learners = shape
    assert norm_ref.BLOCK < E * N < 2 * norm_ref.BLOCK
    case = norm_layouts.big(E, N, 12, learners=learners, seed=73)
    assert case["count"] > case["T"] + 1 and case["steps"] == 12              # the window wraps
    windows = norm_layouts.thirds(case)
    assert len(windows) == 3
    norm, rec, C = _fold_and_check(case, packed_flags, windows)
    assert rec["n_obs"] > 1000 and np.count_nonzero(C) > E                    # episodes are open at the end of the last fold


@pytest.mark.parametrize("packed_flags", [False, True], ids=["rows", "packed"])
@pytest.mark.parametrize("wrapped", [True, False], ids=["count40", "count_steps"])
@pytest.mark.parametrize("steps", norm_layouts.GROUP_STEPS)
def test_windows_around_the_row_groups(steps, wrapped, packed_flags):
    """100 x 3, two learners, T = 24: folds of 7 ... 24 steps -- a full group of fetched rows followed by a ragged one, two and
    three groups -- with a skip, an ended, a done and a parked agent on the rows either side of a group boundary."""
    case = norm_layouts.row_groups(steps, wrapped)
    assert case["steps"] == steps and case["first"] == (40 - steps if wrapped else 0)
    _fold_and_check(case, packed_flags)


@pytest.mark.parametrize("packed_flags", [False, True], ids=["rows", "packed"])
def test_more_partials_than_one_workgroup_has_threads(packed_flags):
    """16 385 x 4 at T = 2: 257 workgroups, the last of 4 columns; the total adds two partials in thread 0."""
    case = norm_layouts.big(16385, 4, 2, seed=74)
    assert -(-16385 * 4 // norm_ref.BLOCK) == 257
    norm, rec, _ = _fold_and_check(case, packed_flags)
    assert rec["n_obs"] > 256 * norm_ref.BLOCK


@pytest.mark.parametrize("F", [7, 10, 1, 16])
def test_other_feature_counts(F):
    case = norm_layouts.big(70, 4, 8, learners=3, F=F)
    norm, rec, _ = _fold_and_check(case, F % 2 == 0, norm_layouts.thirds(case), clip_obs=1.5, clip_reward=0.75)
    assert norm.features == F and rec["mean"].shape == (F,)
    x = norm.obs_ring()
    assert float(x.max()) == 1.5 and float(x.min()) == -1.5 and float(norm.rewards().abs().max()) == 0.75      # the clamp bites


def test_a_batch_without_a_sample_leaves_the_records_bytes_alone():
    case = norm_layouts.make("count_9", 70, 4)
    mid = case["first"] + 2
    L = case["T"] + 1
    for k in range(mid, case["count"]):
        case["skip"][k % L] = 1
    norm, rec, C = _fold_and_check(case, False, [(case["first"], mid)])
    before = _words(norm).copy()
    assert rec["n_obs"] > 0 and np.count_nonzero(C) > 0
    norm.mem.count = case["count"]
    norm.fold_returns()
    norm.fold_obs()
    assert np.array_equal(_words(norm), before)
    assert not norm.carry.cpu().numpy().any()                                 # every re-initialisation row cut its carry


def test_a_nan_is_where_the_reference_has_it_and_nowhere_else():
    # outside the samples: a NaN observation and a NaN reward in a re-initialisation row reach no statistic
    case = norm_layouts.make("two_adjacent_skips", 70, 4)
    L, k = case["T"] + 1, 5
    assert case["skip"][k % L, 0]
    case["obs"][k % L, 0, 1, 2] = np.nan
    case["rew"][k % L, 0, 1] = np.nan
    norm, rec, C = _fold_and_check(case, False)
    assert not np.isnan(norm_ref.words(rec).view(np.float64)).any() and not np.isnan(C).any()
    x, r = norm.obs_ring().cpu().numpy(), norm.rewards().cpu().numpy()
    assert np.isnan(x).sum() == 1 and np.isnan(x[k % L, 0, 1, 2]) and np.isnan(r).sum() == 1 and np.isnan(r[k % L, 0, 1])
    # in a sample: the feature's mean and M2, and the return statistics; the carry does not take it past the episode's end
    case = norm_layouts.make("ended_with_and_without_done", 70, 4)
    k = 6
    assert case["ended"][k % L, 3] and not case["skip"][k % L, 3]
    case["obs"][k % L, 3, 1, 2] = np.nan
    case["rew"][k % L, 3, 1] = np.nan
    norm, rec, C = _fold_and_check(case, True)
    assert np.isnan(rec["mean"][2]) and np.isnan(rec["M2"][2]) and np.isnan(rec["mean"]).sum() == 1
    assert np.isnan(rec["M2_ret"]) and not np.isnan(C).any()
    x = norm.obs_ring().cpu().numpy()
    assert np.isnan(x[..., 2]).all() and not np.isnan(np.delete(x, 2, axis=-1)).any()
    assert np.isnan(norm.rewards().cpu().numpy()).all()


def test_out_may_be_in_and_unaligned_and_ragged_calls():
    case = norm_layouts.big(70, 4, 8, learners=3)
    norm, rec, _ = _fold_and_check(case, False)
    g = torch.Generator().manual_seed(3)
    for rows in (1, 3, 257, 1000):
        pool = (torch.randn(rows * 10 + 8, generator=g) * 3).to(DEV)
        pool[4] = float("nan")
        for start in (0, 1, 2, 4):                                            # 16-byte aligned, and 4, 8 and 16 bytes on
            x = pool[start:start + rows * 10].view(rows, 10)
            want = norm_ref.apply_obs(rec, x.cpu().numpy())
            out = norm.obs(x)
            assert out.data_ptr() != x.data_ptr() and same(out.cpu().numpy(), want), (rows, start)
            y = x.clone()
            assert norm.obs(y, out=y) is y and same(y.cpu().numpy(), want), (rows, start)
            assert int(np.isnan(want).sum()) == (1 if start <= 4 < start + rows * 10 else 0)
    lead = torch.randn((2, 3, 5, 10), generator=g).to(DEV)
    assert same(norm.obs(lead).cpu().numpy(), norm_ref.apply_obs(rec, lead.cpu().numpy()))
    assert norm.obs(torch.zeros((0, 10), device=DEV)).shape == (0, 10)


def test_calls_on_a_side_stream():
    case = norm_layouts.big(70, 4, 8, learners=3, seed=72)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        norm, rec, _ = _fold_and_check(case, False, norm_layouts.thirds(case))
    side.synchronize()
    assert rec["n_obs"] > 0


def test_two_runs_give_identical_bytes():
    case = norm_layouts.big(300, 4, 16, seed=71)
    runs = []
    for _ in range(2):
        norm, _, _ = _fold_and_check(case, False, norm_layouts.thirds(case))
        runs.append([t.clone() for t in (norm._record, norm.carry, norm.obs_ring(), norm.rewards())])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # the apply calls read the record when they run: after another fold the same call gives other bytes
    again = norm.rewards().clone()
    assert torch.equal(again, runs[1][3])
    norm.folded_ret -= 5
    norm.fold_returns()
    assert not torch.equal(norm.rewards(), again)


def test_the_state_dict_restores_record_carry_and_counters():
    case = norm_layouts.big(70, 4, 8, learners=3, seed=76)
    windows = norm_layouts.thirds(case)
    norm, _, _ = _fold_and_check(case, False, windows[:2])
    sd = {k: (v.cpu().clone() if torch.is_tensor(v) else v) for k, v in norm.state_dict().items()}
    full, _, _ = _fold_and_check(case, False, windows)
    mem = norm_layouts.Ring(case, DEV)
    resumed = _normalizer(mem, case["gamma"]).load_state_dict(sd)
    assert resumed.folded_obs == resumed.folded_ret == windows[1][1]
    mem.count = case["count"]
    resumed.fold_returns()
    resumed.fold_obs()
    assert np.array_equal(_words(resumed), _words(full)) and torch.equal(resumed.carry, full.carry)


@pytest.mark.parametrize("packed_flags", [False, True], ids=["rows", "packed"])
def test_live_ring_with_resets(packed_flags):
    """64 envs x 2 agents, step_cap = 5, auto_reset = "agent0_done", T = 8: two rollouts of 8 steps, folded after each; what
    the step launch itself wrote is read back and handed to the reference."""
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    E, N, T = 64, 2, 8
    env = BatchedMultiUAVWorld2D(E, num_agents=N, device=DEV, seed=11)
    mem = DeviceReplay(env, horizon=T, packed_flags=packed_flags)
    mem.begin(env.reset())
    norm = _normalizer(mem, 0.99)
    g = torch.Generator(device=DEV).manual_seed(12)
    rec, C = norm_ref.new_record(10), np.zeros((E, N))
    for rollout in range(2):
        for _ in range(T):
            mem.action_slot().copy_(torch.rand((E, N, 2), generator=g, device=DEV) * 2 - 1)
            mem.step(polar=True, auto_reset="agent0_done", step_cap=5)
        norm.fold_returns()
        norm.fold_obs()
        ring = dict(done=mem.done.cpu().numpy(), learners=N, skip=None if packed_flags else mem.skip.cpu().numpy(),
                    ended=None if packed_flags else mem.ended.cpu().numpy())
        kw = dict(first=rollout * T, count=mem.count, **ring)
        rec = norm_ref.fold_obs(rec, mem.obs.cpu().numpy(), **kw)
        rec, C = norm_ref.fold_returns(rec, C, mem.rew.cpu().numpy(), gamma=0.99, **kw)
        assert norm_ref.same_words(_words(norm), norm_ref.words(rec)) and same(norm.carry.cpu().numpy(), C)
        assert rollout * T * E * N < int(norm.stats.n_obs) < (rollout + 1) * T * E * N
        assert int(norm.stats.n_ret) == int(norm.stats.n_obs)
    sk, _, _ = mem._flags(slice(None), slice(None))
    assert int(sk.sum()) > 0                                                  # resets are in it
    assert same(norm.obs_ring().cpu().numpy(), norm_ref.apply_obs(rec, mem.obs.cpu().numpy()))
    assert same(norm.rewards().cpu().numpy(), norm_ref.scale_rewards(rec, mem.rew.cpu().numpy()))
    with pytest.raises(ValueError, match="overwritten"):
        mem.count += T + 1
        norm.fold_obs()
    env.close()

"""The crafted layouts of tests/key_scan_layouts.py (CPU): every class present where it can exist (recomputed from the
positions), the wavefront plan holding by the host model of the key scan (wavefronts with exactly 0, 1, 6, 7 and all lanes tied,
the tied lane at lane 0 / the last active lane / in the later wavefronts of a workgroup / in an env that straddles two), the
layouts discriminating (the key order alone is wrong for B, B', C, C' and F-tie (a), right for D), and the numpy truth agreeing
with the oracle's observe().  This is what guarantees that tests/test_gpu_key_scan_edges.py reaches the predicate's boundaries,
both near-tie paths and the switch between them."""
import math

import numpy as np
import pytest

import key_scan_layouts as kl
import neighbour_layouts as nl

CASES = [(n, d) for n in kl.AGENTS for d in kl.SENSE]
_cache = {}


def batch(n, d):
    if (n, d) not in _cache:
        _cache[(n, d)] = kl.make_batch(n, d)
    return _cache[(n, d)]


def test_sensing_limits_sit_at_the_top_bottom_and_inside_of_their_buckets():
    assert [int(nl.bits(nl.sq_limit_lt(d))) & 63 for d in kl.SENSE] == [63, 0, 54, 10]
    assert "Ftie-a" in kl.classes_possible(8, 15.0)[1] and "Ftie-a" in kl.classes_possible(8, 9.0)[0]


def test_group_waves_and_lane_mapping():
    assert [kl.group_waves(n) for n in kl.AGENTS] == [3, 3, 1, 2, 1, 3, 1]
    wave, lane = kl.lane_table(70, 6, 3)            # 32 envs per workgroup: env 10 straddles wavefronts 0 and 1
    assert wave[10].tolist() == [0, 0, 0, 0, 1, 1] and lane[10].tolist() == [60, 61, 62, 63, 0, 1]
    assert wave[32, 0] == 3 and lane[32, 0] == 0 and wave[31, 5] == 2 and lane[31, 5] == 63
    wave, lane = kl.lane_table(30, 7, 3)            # 27 envs per workgroup, 3 idle lanes
    assert wave[26, 6] == 2 and lane[26, 6] == 60 and wave[27, 0] == 3
    assert kl.envs_per_group(8, 1, 16) == 8 and kl.envs_per_group(6, 1, 3) == 10


def test_generator_is_deterministic():
    a, b = kl.make_batch(7, 7.3), kl.make_batch(7, 7.3)
    assert np.array_equal(a["loc"], b["loc"]) and np.array_equal(a["vel"], b["vel"]) and list(a["ego_cls"]) == list(b["ego_cls"])
    assert not np.array_equal(kl.make_batch(7, 7.3, seed=1)["loc"], a["loc"])


@pytest.mark.parametrize("n,d_sense", CASES)
def test_every_class_is_present(n, d_sense):
    b = batch(n, d_sense)
    poss, imposs = kl.classes_possible(n, d_sense)
    assert sorted(poss + list(imposs)) == sorted(kl.TIED + kl.UNTIED) and all(imposs.values())   # nothing dropped silently
    seen = {c: 0 for c in kl.TIED + kl.UNTIED}
    for e, i, c in zip(b["ego_env"], b["ego_i"], b["ego_cls"]):
        tags = kl.classify(b["loc"][e], int(i), b["sq_sense"])
        assert c in tags, (e, i, c, tags)
        for t in tags:
            seen[t] += 1
    for c in poss:
        assert seen[c] >= 4, (c, seen)
    for c in imposs:
        assert seen[c] == 0, (c, seen)
    # class I sweeps the ego index
    sweep = {int(i) for i, c in zip(b["ego_i"], b["ego_cls"]) if c == "I"}
    assert sweep == {0, 1, n - 2, n - 1}


@pytest.mark.parametrize("n,d_sense", CASES)
def test_wavefront_plan_holds_by_the_model(n, d_sense):
    b = batch(n, d_sense)
    W, epw, loc, sq = b["W"], b["epw"], b["loc"], b["sq_sense"]
    E = loc.shape[0]
    cnt = kl.check_plan(b)                                         # the model's count of every wavefront == the plan
    assert np.array_equal(cnt, kl.tied_lanes_per_wave(loc, n, d_sense, W))
    act = kl.active_lanes_per_wave(E, n, W)
    assert {0, 1, 6, 7} <= set(cnt.tolist()) and (cnt[act > 0] == act[act > 0]).any()
    assert E % epw != 0 or n == 64                                 # a ragged last workgroup (one env per workgroup at 64)
    if n == 8:
        assert len(cnt) % 2 == 0                                   # pairs of tiles take an even number of wavefronts
    tie = kl.near_tie(loc, sq)
    wave, lane = kl.lane_table(E, n, W)
    kinds = b["plan"]
    for w, kind in kinds.items():
        lanes = np.sort(lane[(wave == w) & tie])
        if kind == "first":
            assert lanes.tolist() == [0]
        if kind == "last":
            assert lanes.tolist() == [lane[wave == w].max()]
        if kind == "pair":
            e = np.unique(np.nonzero((wave == w) & tie)[0])
            assert len(e) == 1 and len(lanes) == 2                 # two tied lanes inside one env
    # only crafted egos (and polygon lanes) tie, and every tied class ego does
    crafted = np.zeros((E, n), bool)
    for e, i, c in zip(b["ego_env"], b["ego_i"], b["ego_cls"]):
        crafted[e, i] = c in kl.TIED
    crafted[b["poly_envs"]] = True
    assert np.array_equal(tie, crafted)
    # B, C and F-tie (a) on the per-lane path (1..6 tied lanes) and on the whole-wave path (>= 7)
    want = [c for c in ("B", "C", "Ftie-a") if c in kl.classes_possible(n, d_sense)[0]]
    for c in want:
        at = cnt[b["ego_wave"][b["ego_cls"] == c]]
        assert ((at >= 1) & (at <= 6)).any() and (at >= 7).any(), (c, at)
    if n == 64:                                                    # ranks up to 62, winners beyond lane 62's slot
        tj, _ = kl.truth(loc, sq)
        assert tj[tie].max() == 63 and (b["ego_i"][np.isin(b["ego_cls"], kl.TIED)] == 63).any()
    if W > 1:
        tied_ego = np.isin(b["ego_cls"], kl.TIED)
        assert {1, W - 1} <= set((b["ego_wave"][tied_ego] % W).tolist())
        # an env whose lanes straddle two wavefronts: the tied ego in the later one with a winner in the earlier one, and reverse
        tj, _ = kl.truth(loc, sq)
        later = earlier = 0
        for e, i in zip(b["ego_env"][tied_ego], b["ego_i"][tied_ego]):
            for j in tj[e, i]:
                if j >= 0:
                    later += wave[e, j] < wave[e, i]
                    earlier += wave[e, j] > wave[e, i]
        assert later > 0 and earlier > 0


@pytest.mark.parametrize("n,d_sense", CASES)
def test_layouts_discriminate(n, d_sense):
    """Where the fallback is needed the key order alone gives another answer than the (root, slot) order; for D it gives the same
    and the predicate is false."""
    b = batch(n, d_sense)
    loc, sq = b["loc"], b["sq_sense"]
    kp, (tj, _), tie = kl.key_path(loc, sq), kl.truth(loc, sq), kl.near_tie(loc, sq)
    hit = {c: 0 for c in ("B", "B'", "C", "C'", "Ftie-a", "Ftie-a'", "D12", "D23")}
    for e, i, c in zip(b["ego_env"], b["ego_i"], b["ego_cls"]):
        if c in ("B", "B'", "C", "C'", "Ftie-a", "Ftie-a'"):
            assert tie[e, i] and not np.array_equal(kp[e, i], tj[e, i]), (e, i, c)
            hit[c] += 1
        if c in ("D12", "D23"):
            assert not tie[e, i] and np.array_equal(kp[e, i], tj[e, i]), (e, i, c)
            hit[c] += 1
    assert all(v >= 4 for c, v in hit.items() if c in kl.classes_possible(n, d_sense)[0]), hit
    assert np.array_equal(kp[~tie], tj[~tie])                      # the model's claim: no near tie -> the key order is the truth


@pytest.mark.parametrize("n,d_sense", CASES)
def test_truth_matches_nearest_two_and_the_oracle(oracle_mod, n, d_sense):
    b = batch(n, d_sense)
    loc, vel, sq = b["loc"], b["vel"], b["sq_sense"]
    E = loc.shape[0]
    tj, td = kl.truth(loc, sq)
    some = list(zip(b["ego_env"], b["ego_i"])) + [(int(e), 0) for e in b["poly_envs"][:4]]
    for e, i in some:                                              # the vectorised truth IS neighbour_layouts.nearest_two
        ref = nl.nearest_two(loc[e], int(i), sq)
        assert [j for j in tj[e, i] if j >= 0] == [j for j, _ in ref], (e, i)
        assert [d for d in td[e, i] if np.isfinite(d)] == [d for _, d in ref], (e, i)
    orc = oracle_mod.OracleMulti(num_envs=E, num_agents=n, d_sense=d_sense, nthreads=8, **kl.WORLD)
    orc.reset_philox(1)
    orc.set_state(loc=loc, vel=vel)
    obs = orc.observe()
    theta = np.arctan2(vel[..., 1], vel[..., 0])
    ds = np.float32(d_sense)
    for k in range(2):
        j, d = tj[..., k], td[..., k]
        has = j >= 0
        h = np.take_along_axis(theta, np.maximum(j, 0), 1) - theta
        want_h = np.where(has, np.arctan2(np.sin(h), np.cos(h)) / math.pi, 0.0)
        want_d = np.where(has, (np.where(has, d, 0).astype(np.float32) / ds).astype(np.float64), 1.0)
        assert np.abs(obs[..., 6 + 3 * k] - want_h).max() < 1e-9, k   # identity, through the heading column
        assert np.abs(obs[..., 4 + 3 * k] - want_d).max() <= 1e-5, k
    # headings are distinct: a wrong neighbour moves a heading column by at least 1.2 / n
    dth = np.abs(theta[:, :, None] - theta[:, None, :])
    dth = np.minimum(dth, 2 * np.pi - dth) / np.pi + np.eye(n)[None] * 9
    assert dth.min() > 1.2 / n - 1e-9

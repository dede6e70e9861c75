"""The crowded reset cases of tests/reset_layouts.py (CPU): the numpy restatement of the candidate stream and of the sequential
accept / reject chain equals the oracle bit for bit on every case, world, seed and episode index that
tests/test_gpu_reset_crowded.py reaches; no slot needs more than MAX_ATTEMPTS candidates on any of them (a CONDITION: it bounds the
device's redraw loops, so it has to hold before anything runs on a GPU -- a case that breaks it gets a larger box, the cap stays);
the events the device's bookkeeping has to survive -- third and fifth candidates, a redraw that makes or frees a clash of a
higher slot, bodies against learners, a target against its own start, a clash found in the last partial trip of the clash loop --
are present in numbers; and the accepted layouts are legal."""
import numpy as np
import pytest

import reset_layouts as rl

NAMES = [c.name for c in rl.CROWDED]
_primary = {}


def primary(case):
    """Episode 0 of the case as created: what the coverage conditions are stated on."""
    if case.name not in _primary:
        _primary[case.name] = rl.draw_layouts(case, rl.worlds(case)[0], case.seed, 0)
    return _primary[case.name]


def schedule(case):
    """(world, seed) pairs the GPU tests run a case on: as created, after the seed change, after the world change that follows."""
    w1, w2 = rl.worlds(case)
    return [(w1, case.seed), (w1, case.seed2), (w2, case.seed2)]


def _oracle(oracle_mod, case, world):
    kw = rl.env_kwargs(case)
    kw.update(x_size=world["x_size"], y_size=world["y_size"])
    orc = oracle_mod.OracleMulti(num_envs=case.E, nthreads=8, **kw)
    if world["levels"]:
        orc.set_curriculum(world["levels"], *world["window"])
    return orc


def test_numpy_philox_against_the_oracle(oracle_mod):
    rng = np.random.default_rng(1)
    ctr = rng.integers(0, 2 ** 32, size=(300, 4), dtype=np.uint64)
    ctr[:100, 1] = (ctr[:100, 1] & 0xFFFF0000) | rng.integers(1, 2 ** 16, size=100, dtype=np.uint64)   # env bits 32-47 beside the slot
    ctr[100:110, 1] |= 0xFFFF
    ctr[110:120] = [0, 0, 0, 0]
    ctr[120:130] = 0xFFFFFFFF
    key = rng.integers(0, 2 ** 32, size=(300, 2), dtype=np.uint64)
    for k in range(300):
        got = rl.philox4x32_10(ctr[k, 0], ctr[k, 1], ctr[k, 2], ctr[k, 3], int(key[k, 0]), int(key[k, 1]))
        assert [int(g) for g in got] == oracle_mod.philox4x32(ctr[k], key[k]).tolist(), (ctr[k], key[k])
    # vectorised over counters == one at a time
    vec = rl.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], 0xDEADBEEF, 0x12345678)
    one = [oracle_mod.philox4x32(ctr[k], [0xDEADBEEF, 0x12345678]) for k in range(300)]
    np.testing.assert_array_equal(np.stack(vec, axis=-1), np.stack(one))
    # reset_words packs a 48-bit env id: bits 32-47 into the low half of word 1
    ge = np.array([rl.BIG_OFFSET + 5, 0xABCD00000007, 9], dtype=np.uint64)
    w = rl.reset_words(ge, 0x2A, 3, 6, 0x1122334455)
    for k, g in enumerate(ge.tolist()):
        want = oracle_mod.philox4x32([g & 0xFFFFFFFF, ((g >> 32) & 0xFFFF) | (0x2A << 16), 3, 6], [0x22334455, 0x11])
        assert [int(x[k]) for x in w] == want.tolist()


def test_case_table():
    assert len(set(NAMES)) == len(NAMES)
    assert sum(c.env_offset == rl.BIG_OFFSET for c in rl.CROWDED) >= 2 and any(c.env_offset < 2 ** 17 for c in rl.CROWDED)
    assert all(500 <= c.E <= 1100 for c in rl.CROWDED)
    assert 2 * sum(c.E % 64 != 0 for c in rl.CROWDED) >= len(rl.CROWDED)
    shapes = {(c.L, c.B) for c in rl.CROWDED}
    assert {(2, 0), (4, 0), (5, 0), (8, 0), (13, 0), (24, 0), (64, 0), (3, 5), (8, 16), (24, 40)} <= shapes
    lv = rl.BY_NAME["levels"].levels
    assert lv[rl.CHAIN_FREE_LEVEL]["n_active"] == 1 and lv[rl.CHAIN_FREE_LEVEL]["b_active"] == 0
    assert len({(l["n_active"], l["b_active"]) for l in lv}) == len(lv)


def _legal(case, world, lay, ctx):
    table = world["levels"] or [dict(x_size=world["x_size"], y_size=world["y_size"], collider_radius=world["collider_radius"])]
    half = np.array([[l["x_size"] / 2.0, l["y_size"] / 2.0] for l in table])[lay["level"]]                  # [E, 2]
    two_r = np.array([np.float32(2 * l["collider_radius"]) for l in table], np.float32)[lay["level"]][:, None, None]
    start = np.concatenate([lay["loc"], lay["body"][:, :, :2]], axis=1)
    on = np.isfinite(start[..., 0])
    assert np.array_equal(on, lay["attempts"][..., 0] > 0), ctx
    assert (np.abs(start)[on] <= np.repeat(half[:, None, :], start.shape[1], axis=1)[on]).all(), ctx + ": a start point outside the box"
    assert (np.abs(lay["tgt"]) <= half[:, None, :]).all(), ctx + ": a target outside the box"
    with np.errstate(invalid="ignore"):
        s = rl.too_close(two_r, start[:, :, None, 0], start[:, :, None, 1], start[:, None, :, 0], start[:, None, :, 1])
        lon = lay["flags"] == 0
        t = rl.too_close(two_r, lay["tgt"][:, :, None, 0], lay["tgt"][:, :, None, 1], lay["tgt"][:, None, :, 0], lay["tgt"][:, None, :, 1])
        own = rl.too_close(two_r[:, :, 0], lay["tgt"][..., 0], lay["tgt"][..., 1], lay["loc"][..., 0], lay["loc"][..., 1])
    off = ~np.eye(start.shape[1], dtype=bool)[None]
    assert not (s & off & on[:, :, None] & on[:, None, :]).any(), ctx + ": two start points within 2R"
    offl = ~np.eye(case.L, dtype=bool)[None]
    assert not (t & offl & lon[:, :, None] & lon[:, None, :]).any(), ctx + ": two targets within 2R"
    assert not (own & lon).any(), ctx + ": a target within 2R of its own start"


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_oracle_bounded_and_legal(oracle_mod, name):
    """Every (world, seed) of the schedule, every episode index 0 .. EPISODES - 1: the oracle is reset, then driven through
    step_ex with a step cap of 1 (one call ends every episode, the next re-initialises every env with the next episode index)."""
    case = rl.BY_NAME[name]
    worst = 0
    for wi, (world, seed) in enumerate(schedule(case)):
        orc = _oracle(oracle_mod, case, world)
        zeros = np.zeros((case.E, case.L, 2))
        for ep in range(rl.EPISODES):
            if ep == 0:
                orc.reset_philox(seed, env_offset=case.env_offset)
            else:
                orc.step_ex(zeros, reset_policy=1, step_cap=1, seed=seed, env_offset=case.env_offset)
                rm = orc.step_ex(zeros, reset_policy=1, step_cap=1, seed=seed, env_offset=case.env_offset)[3]
                assert rm.all()
            assert (orc.counters[:, 3] == ep + 1).all()
            ctx = f"case {name} world {wi} seed {seed} episode {ep}"
            if wi == 0 and ep == 0:
                lay = primary(case)
            else:
                lay = rl.draw_layouts(case, world, seed, ep, pairs=False)        # raises Unbounded past MAX_ATTEMPTS candidates
            worst = max(worst, int(lay["attempts"].max()))
            np.testing.assert_array_equal(lay["level"], orc.level, err_msg=ctx)
            np.testing.assert_array_equal(lay["flags"], orc.flags, err_msg=ctx)
            np.testing.assert_array_equal(lay["loc"], orc.loc.astype(np.float32), err_msg=ctx)
            np.testing.assert_array_equal(lay["tgt"], orc.tgt.astype(np.float32), err_msg=ctx)
            np.testing.assert_array_equal(lay["init_d"], orc.init_d.astype(np.float32), err_msg=ctx)
            np.testing.assert_array_equal(lay["init_d"], orc.prev_d.astype(np.float32), err_msg=ctx)
            assert (orc.loc.astype(np.float32) == orc.loc).all() and (orc.vel == 0).all()
            if case.B:
                np.testing.assert_array_equal(lay["body"], orc.body, err_msg=ctx)
            _legal(case, world, lay, ctx)
    assert worst <= rl.MAX_ATTEMPTS, f"case {name}: a slot took {worst} candidates"
    print(f"case {name}: most candidates of one slot over the schedule: {worst}")


@pytest.mark.parametrize("name", NAMES)
def test_events_are_present(name):
    case = rl.BY_NAME[name]
    lay = primary(case)
    n = {k: int(lay[k].sum()) for k in rl.EVENTS}
    att = lay["attempts"][..., 0]
    msg = f"case {name} (E = {case.E}): {n}, candidates per start slot: mean {att[att > 0].mean():.2f}, max {att.max()}"
    print(msg)
    assert n["deep"] >= 0.30 * case.E and n["deeper"] >= 0.05 * case.E, msg
    if case.L + case.B >= 5:
        for k in ("set_bit", "clear_bit", "own_start", "tail_trip"):
            assert n[k] >= 20, msg
    if case.B:
        assert n["body_vs_learner"] >= 20, msg
    # several envs of one wavefront redraw side by side (each with its own lowest clashing slot; the ones that finish early sit
    # out the later rounds with no clash at all); with levels, envs that never redraw share wavefronts with ones that do
    g = rl.envs_per_wave(case)
    if g > 1:
        redraws = (lay["attempts"] > 1).any(axis=(1, 2))[:case.E // g * g].reshape(-1, g)
        mixed = int((redraws.any(axis=1) & ~redraws.all(axis=1)).sum())
        several = int((redraws.sum(axis=1) >= 2).sum())
        assert several >= 20, f"{msg}; wavefronts with two or more redrawing envs: {several}"
        if name == "levels":
            assert mixed >= 20, f"{msg}; wavefronts with a clash-free env next to a redrawing one: {mixed}"


def test_curriculum_mixes_a_chain_free_level_with_jammed_ones():
    case = rl.BY_NAME["levels"]
    for world, seed in schedule(case)[::2]:
        lo, hi = world["window"]
        levels = np.concatenate([rl.draw_levels(world, np.uint64(case.env_offset) + np.arange(case.E, dtype=np.uint64),
                                                np.full(case.E, ep, np.uint32), seed) for ep in range(3)])
        assert set(np.unique(levels)) == set(range(lo, hi + 1)), (world["window"], np.bincount(levels))
    lay = primary(case)
    assert set(np.unique(lay["level"])) == set(range(len(case.levels))), np.bincount(lay["level"])
    g = rl.envs_per_wave(case)
    lv = lay["level"][:case.E // g * g].reshape(-1, g)
    jam = (lay["attempts"] >= 3).any(axis=(1, 2))[:case.E // g * g].reshape(-1, g)
    mixed = int(((lv == rl.CHAIN_FREE_LEVEL).any(axis=1) & jam.any(axis=1)).sum())
    assert g >= 4 and mixed >= 50, f"groups of {g} consecutive envs with the chain-free level beside a jammed env: {mixed} of {len(lv)}"
    free = lay["attempts"][lay["level"] == rl.CHAIN_FREE_LEVEL]
    assert (free[:, 0, 0] == 1).all() and (free[:, 1:] == 0).all()      # one start candidate, nobody else: only its target can redraw

"""Cross-check of the oracle against the REFERENCE ITSELF, beyond the parity fixtures: several agent counts and seeds,
three episodes per world, random and goal-seeking commands, evaluate flags and float64-position episodes.  The reference's
side of every scenario is recorded in tests/golden/live_*.npz (tests/golden/make_live_golden.py drives the reference with
exactly these scenarios); the oracle is run live here and must reproduce it bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from golden_util import load_fixture, tie_agents  # noqa: E402
from make_live_golden import F64_CASES, MUW_CASES, UW_SEEDS, muw_kwargs, signed_zero_state  # noqa: E402


def _check_multi_step(orc, ref, t, o_obs, o_rew, o_done, ctx, exact_rew=True):
    np.testing.assert_array_equal(o_done[0], ref["done"][t], err_msg=ctx)
    np.testing.assert_array_equal(orc.loc[0], ref["loc"][t], err_msg=ctx)
    np.testing.assert_array_equal(orc.vel[0], ref["vel"][t], err_msg=ctx)
    np.testing.assert_array_equal(orc.prev_d[0], ref["prev_d"][t], err_msg=ctx)
    np.testing.assert_array_equal(orc.flags[0], ref["flags"][t], err_msg=ctx)
    np.testing.assert_array_equal(orc.counters[0, :3], ref["counters"][t], err_msg=ctx)
    if exact_rew:
        np.testing.assert_array_equal(o_rew[0], ref["rew"][t], err_msg=ctx)
    else:
        np.testing.assert_allclose(o_rew[0], ref["rew"][t], rtol=1e-6, atol=1e-6, err_msg=ctx)


@pytest.mark.parametrize("n,seed", MUW_CASES)
def test_oracle_equals_live_reference(oracle_mod, n, seed):
    ref, meta = load_fixture(f"live_muw_n{n}_s{seed}")
    assert meta["kwargs"] == muw_kwargs(n, seed)
    orc = oracle_mod.OracleMulti(num_envs=1, **muw_kwargs(n, seed))
    g = oracle_mod.MTStream(seed)
    T = meta["T"]
    for episode in range(meta["episodes"]):
        orc.reset_mt(g)
        np.testing.assert_array_equal(orc.observe()[0], ref["reset_obs"][episode])
        for t in range(T):
            k = episode * T + t
            o_obs, o_rew, o_done = orc.step(ref["actions"][k], evaluate=bool(t % 7 == 0))
            ctx = f"n={n} seed={seed} ep={episode} t={t}"
            _check_multi_step(orc, ref, k, o_obs, o_rew, o_done, ctx)
            np.testing.assert_array_equal(o_obs[0], ref["obs"][k], err_msg=ctx)


@pytest.mark.parametrize("seed", UW_SEEDS)
def test_oracle_uw_equals_live_reference(oracle_mod, seed):
    ref, meta = load_fixture(f"live_uw_s{seed}")
    orc = oracle_mod.OracleSingle(num_envs=1)
    g = oracle_mod.MTStream(seed)
    rng = np.random.default_rng(seed)
    T = meta["T"]
    for episode in range(meta["episodes"]):
        orc.reset_mt(g)
        np.testing.assert_array_equal(orc.observe()[0], ref["reset_obs"][episode])
        for t in range(T):
            k = episode * T + t
            a = rng.uniform(-12, 12, 2).astype(np.float32) if (t + seed) % 2 else rng.uniform(-12, 12, 2)
            o_obs, o_rew, o_done, o_info = orc.step(a)
            assert bool(o_done[0]) == bool(ref["done"][k]) and o_rew[0] == ref["rew"][k] and o_info[0] == ref["distance"][k]
            np.testing.assert_array_equal(o_obs[0], ref["obs"][k])
            np.testing.assert_array_equal(orc.loc[0], ref["loc"][k])
            np.testing.assert_array_equal(orc.vel[0], ref["vel"][k])


@pytest.mark.parametrize("n,circular", F64_CASES)
def test_oracle_float64_episodes_equal_live_reference(oracle_mod, n, circular):
    """Float64-position episodes of the reference: reset(circular=True) (MUW:157-163), and a random reset
    followed by the plotting script's float64 pokes of location / target_location
    (test_sac_multi_plot_trajectory.py:43-49; init / prev distance stay the stale float32 scalars).  State and masks
    bit for bit; in the poke pattern the reward may differ in the last float32 digit (NEP 50 evaluates
    1.5*np.float32(init_distance) in float32 there; the oracle keeps no scalar dtypes)."""
    ref, meta = load_fixture(f"live_f64_n{n}_{'circular' if circular else 'poked'}")
    orc = oracle_mod.OracleMulti(num_envs=1, num_agents=n)
    g = oracle_mod.MTStream(300 + n)
    orc.reset_mt(g, circular=circular)
    if not circular:
        orc.loc[0] = ref["poked_loc"]
        orc.tgt[0] = ref["poked_tgt"]
        orc.f64pos[:] = 1
    else:
        np.testing.assert_array_equal(orc.observe()[0], ref["reset_obs"])
    assert int(orc.f64pos[0]) == 1
    for t in range(meta["T"]):
        o_obs, o_rew, o_done = orc.step(ref["actions"][t], evaluate=bool(t % 11 == 0))
        ctx = f"n={n} circular={circular} t={t}"
        _check_multi_step(orc, ref, t, o_obs, o_rew, o_done, ctx, exact_rew=circular)
        # neighbour columns of exactly tied agents depend on numpy's argsort tie order (platform dependent)
        ties = tie_agents(ref["loc"][t], 15, True)
        got, want = o_obs[0].copy(), ref["obs"][t].copy()
        got[ties, 4:] = 0; want[ties, 4:] = 0
        np.testing.assert_array_equal(got, want, err_msg=ctx)
    assert int(orc.counters[0, 1]) > 0, "nobody reached a target: scenario too short"


def test_oracle_signed_zero_angles_equal_live_reference(oracle_mod):
    """Velocities, target offsets and neighbour offsets of (+-0, +-0), a done agent among them: the oracle's observation
    equals the reference's recorded one bit for bit, so it follows math.atan2 on signed zeros (atan2(+0, -0) = pi,
    atan2(-0, -0) = -pi) and can judge the device kernels there."""
    ref, meta = load_fixture("live_signed_zero")
    assert ref["obs"][0, 0, 1] == 1.0 and ref["obs"][1, 0, 1] == -1.0
    for k in range(meta["cases"]):
        loc, vel, tgt, done = signed_zero_state(k)
        orc = oracle_mod.OracleMulti(num_envs=1, num_agents=4)
        orc.set_state(loc=loc, vel=vel, tgt=tgt, flags=done)
        np.testing.assert_array_equal(orc.observe()[0], ref["obs"][k], err_msg=f"case {k}")

"""step_kernel reads the parameters of its straight-line path from fixed byte offsets of its argument segment
(fetch_step_args, csrc/uavx_multi_step.hpp): a wrong, swapped or shifted offset must not hide behind default values that
happen to be equal, or behind a comparison no run ever decides.

17 envs (a partial last wavefront) x N for the compile-time variants 1, 2, 4, 5, 8, the runtime-N variant (3) and one shape with
scripted bodies (the variant that keeps the compiler-placed loads), 40 steps against oracle.OracleMulti with the comparison of
tests/test_gpu_parity.py: masks, flags, counters, float32 positions and float64 velocities bit-exact, observations and rewards
within 1e-5.  Every fetched parameter is moved off the base world ONE AT A TIME -- tau (0.05, and 2^-1030, whose reciprocal
overflows so that uavx_create has to clear recip_ok and the kernel divides; see VARIANTS), acceleration and speed limit, sensing range,
collider radius, a box with x_size != y_size --, evaluate is run as 0 and as 1 (out-of-bounds is the one `done` it decides)
and the commands as float32 and float64.  The base world is small and fast (12 m box, 2R = 1.4 m apart from
the 1 m hard-collision limit, d_sense = 4 m, 150 m/s^2 so that the 12 m/s speed limit binds too): on the oracle's side the 40 steps
of the 4-UAV base run hold 355 out-of-bounds `done`s (none with evaluate), 22 hard collisions and 1 500 sensed neighbours, and
the tau = 0.05 runs add arrivals."""
import numpy as np
import pytest

from golden_util import obs_err
from test_gpu_parity import TOL, _check_multi_state, _np

pytestmark = pytest.mark.gpu

E, T = 17, 40
BASE = dict(x_size=12.0, y_size=12.0, max_speed=12.0, max_acceleration=150.0, collider_radius=0.7, d_sense=4.0)
SHAPES = [(1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (8, 0), (4, 4)]          # (UAVs, scripted bodies)
VARIANTS = {
    "base": {},
    "tau_0.05": dict(tau=0.05),
    # 1/tau overflows: the only kind of step size uavx_create's check rejects (with an exact reciprocal and no overflow the
    # Markstein form is the IEEE quotient).  The acceleration limit goes up with it so that the velocities (a_max tau per step)
    # stay float32 normals: the heading is taken from the float32 velocity, and a pair flushed to (0, 0) has none to compare
    "tau_no_reciprocal": dict(tau=2.0 ** -1030, max_acceleration=2.0 ** 1000),
    "max_acceleration": dict(max_acceleration=60.0),
    "max_speed": dict(max_speed=7.0),
    "d_sense": dict(d_sense=2.5),
    "collider_radius": dict(collider_radius=0.3),
    "x_ne_y": dict(x_size=16.0, y_size=9.0),
    "evaluate": dict(evaluate=True),
    "float64_commands": dict(f64=True),
}


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import gym_uav_collision_avoidance_amd as pkg
    return pkg


def actions(rng, orc, t, vmax, f64):
    """Every third env brakes towards its targets (arrivals: the 0.5 m / 0.2 m/s test and the finish); the others hold a random
    command for eight steps at a time, which carries them into each other and out of the box."""
    n = orc.loc.shape[1]
    if t % 8 == 0:
        actions.held = rng.uniform(-vmax, vmax, size=(E, n, 2))
    act = actions.held.copy()
    seek = np.arange(E) % 3 == 0
    act[seek] = 2.0 * (orc.tgt - orc.loc).reshape(E, n, 2)[seek]
    return act.astype(np.float64 if f64 else np.float32)


def worlds(n, bodies, variant):
    v = dict(VARIANTS[variant])
    opts = dict(evaluate=v.pop("evaluate", False), f64=v.pop("f64", False), tau=v.pop("tau", 0.02))
    kw = dict(BASE, num_agents=n, **v)
    if bodies:
        kw.update(num_bodies=bodies, body_period=8, body_seed=3)
    return kw, opts


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n,bodies", SHAPES)
def test_step_reads_every_parameter_from_its_own_place(amd, oracle_mod, n, bodies, variant):
    kw, opts = worlds(n, bodies, variant)
    seed = 40 + n
    env = amd.BatchedMultiUAVWorld2D(E, seed=seed, **kw)
    if opts["tau"] != env.tau:
        env.tau = opts["tau"]
        env.set_config()               # re-derives tau, rtau and recip_ok
    orc = oracle_mod.OracleMulti(num_envs=E, tau=opts["tau"], **kw)
    obs_g = env.reset()
    orc.reset_philox(seed)
    assert obs_err(_np(obs_g), orc.observe()) <= TOL
    rng = np.random.default_rng(7 * n + bodies)
    for t in range(T):
        act = actions(rng, orc, t, kw["max_speed"], opts["f64"])
        obs_g, rew_g, done_g, _ = env.step(act, evaluate=opts["evaluate"])
        obs_o, rew_o, done_o = orc.step(act, evaluate=opts["evaluate"])
        ctx = f"{n}+{bodies} {variant} step {t}"
        np.testing.assert_array_equal(_np(done_g).astype(np.uint8), done_o, err_msg=ctx)
        ref = orc.get_state()
        _check_multi_state(env, dict(flags=ref["flags"], loc=ref["loc"], prev_d=ref["prev_d"], vel=ref["vel"],
                                     counters=ref["counters"][:, :3]), ctx)
        e_obs, e_rew = obs_err(_np(obs_g), obs_o), float(np.abs(_np(rew_g) - rew_o).max())
        print(f"{ctx}: obs err {e_obs:.3g} rew err {e_rew:.3g}")
        assert e_obs <= TOL and e_rew <= TOL, f"{ctx}: obs err {e_obs:.3g}, rew err {e_rew:.3g}"
    env.close()

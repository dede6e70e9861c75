"""The 4-UAV one-step kernel stores positions and rewards as quad-packed 16-byte rows (csrc/uavx_multi_step.hpp, UAVX_PACKWT):
even lanes write {x0, y0, x1, y1}, the first lane of every quad writes the env's four rewards.  A row must never reach past its
array, a partial last wavefront must drop its idle quads, and a caller-owned reward array that does not start on a 16-byte
boundary must get the dword stores it always got.

Plain `step`, N = 4, against the CPU oracle at the batch sizes where the row logic can go wrong:
    E = 1   one live quad among fifteen idle ones        E = 15  a partial last wavefront
    E = 16  an exact wavefront                            E = 17  two workgroups, one quad in the second
    E = 33  three workgroups
64 steps of seeded polar commands (a noisy speed along a noisy bearing to the target, handed over as the velocity command
`step` takes), float32 and float64 actions, in a world small enough for collisions and arrivals to set flags.  State and dones bit for
bit, rewards and observations at the parity tests' 1e-5.

The Python layer does not refuse a reward tensor that is only 4-byte aligned (it checks the observation pointer alone), so the
unaligned case runs the kernel's dword fallback and is compared bit for bit with the aligned run."""
import numpy as np
import pytest

from golden_util import obs_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
N = 4
STEPS = 64
KW = dict(x_size=12.0, y_size=10.0, num_agents=N, d_sense=9.0, collider_radius=0.5)   # small box: collisions, arrivals
REW_SENTINEL = -12345.0
DONE_SENTINEL = 0xA5


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import gym_uav_collision_avoidance_amd as pkg
    return pkg


def _np(t):
    return t.detach().cpu().numpy()


def _commands(rng, orc, dtype):
    """Polar commands -- speed 0.2 .. 3 x the distance to the target, heading its bearing + N(0, 0.4 rad) -- as the velocity
    commands `step` takes (the oracle's state is the device's bit for bit, so both see the same command)."""
    d = orc.tgt - orc.loc
    v = np.hypot(d[..., 0], d[..., 1]) * rng.uniform(0.2, 3.0, size=d.shape[:2])
    th = np.arctan2(d[..., 1], d[..., 0]) + rng.normal(0.0, 0.4, size=d.shape[:2])
    return np.stack([v * np.cos(th), v * np.sin(th)], axis=-1).astype(dtype)


def _pair(amd, oracle_mod, E, seed):
    env = amd.BatchedMultiUAVWorld2D(E, seed=seed, env_offset=7, **KW)
    orc = oracle_mod.OracleMulti(num_envs=E, nthreads=4, **KW)
    env.reset()
    orc.reset_philox(seed, mask=None, env_offset=7)
    return env, orc


def _check_against_oracle(env, orc, got, want, ctx):
    obs_g, rew_g, done_g = got
    obs_o, rew_o, done_o = want
    np.testing.assert_array_equal(_np(done_g).astype(np.uint8), done_o, err_msg=ctx + " dones")
    ref = orc.get_state()
    st = {k: _np(v) for k, v in env.get_state().items()}
    np.testing.assert_array_equal(st["loc"], ref["loc"].astype(np.float32), err_msg=ctx + " loc")
    np.testing.assert_array_equal(st["vel"], ref["vel"], err_msg=ctx + " vel")
    np.testing.assert_array_equal(st["flags"], ref["flags"], err_msg=ctx + " flags")
    e_obs = obs_err(_np(obs_g), obs_o)
    e_rew = float(np.abs(_np(rew_g) - rew_o).max())
    assert e_obs <= TOL and e_rew <= TOL, f"{ctx}: obs err {e_obs:.3g}, rew err {e_rew:.3g}"


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("E", [1, 15, 16, 17, 33])
def test_packed_rows_against_oracle(amd, oracle_mod, E, dtype):
    import torch
    env, orc = _pair(amd, oracle_mod, E, seed=4100 + E)
    rng = np.random.default_rng(100 * E + (dtype is np.float64))
    for t in range(STEPS):
        act = _commands(rng, orc, dtype)
        ev = bool(t % 5 == 4)
        # (a float32 device tensor takes the host layer's fast path, everything else the checked one: both write the
        #  internal double-buffered outputs)
        got = env.step(torch.from_numpy(act).to(env.device) if dtype is np.float32 else act, evaluate=ev)[:3]
        want = orc.step(act, evaluate=ev)
        _check_against_oracle(env, orc, got, want, f"E={E} {np.dtype(dtype).name} step {t}")
    assert orc.flags.any() or E == 1, "the batch must set flags (collisions, arrivals)"
    env.close()


class _Embedded:
    """Reward and done storage of one env inside larger buffers with sentinel cells in front and behind.  `lead` floats in
    front of the rewards: 4 -> the array starts on a 16-byte boundary, 1 -> 4-byte aligned only."""

    def __init__(self, env, E, lead):
        import torch
        self.big_r = torch.full((lead + E * N + 7,), REW_SENTINEL, dtype=torch.float32, device=env.device)
        self.big_d = torch.full((16 + E * N + 16,), DONE_SENTINEL, dtype=torch.uint8, device=env.device)
        assert self.big_r.data_ptr() % 16 == 0 and self.big_d.data_ptr() % 16 == 0
        self.lead, self.n = lead, E * N
        self.rew = self.big_r[lead:lead + E * N].view(E, N)
        self.done = self.big_d[16:16 + E * N].view(E, N)
        self.obs = torch.empty((E, N, 10), dtype=torch.float32, device=env.device)
        assert self.rew.is_contiguous() and self.rew.data_ptr() % 16 == (4 * lead) % 16

    def out(self):
        return (self.obs, self.rew, self.done)

    def check_sentinels(self, ctx):
        r, d = _np(self.big_r), _np(self.big_d)
        assert (r[:self.lead] == REW_SENTINEL).all() and (r[self.lead + self.n:] == REW_SENTINEL).all(), ctx + ": reward sentinel overwritten"
        assert (d[:16] == DONE_SENTINEL).all() and (d[16 + self.n:] == DONE_SENTINEL).all(), ctx + ": done sentinel overwritten"


def test_caller_owned_aligned_rows_stay_inside_their_array(amd, oracle_mod):
    E = 17
    env, orc = _pair(amd, oracle_mod, E, seed=4200)
    emb = _Embedded(env, E, lead=4)
    rng = np.random.default_rng(17)
    for t in range(STEPS):
        act = _commands(rng, orc, np.float32)
        obs, rew, done, _ = env.step(act, out=emb.out())
        assert rew.data_ptr() == emb.rew.data_ptr() and done.data_ptr() == emb.done.data_ptr()
        ctx = f"aligned out= step {t}"
        emb.check_sentinels(ctx)
        _check_against_oracle(env, orc, (obs, rew, done), orc.step(act, evaluate=False), ctx)
    env.close()


def test_caller_owned_unaligned_rewards_equal_the_aligned_run(amd, oracle_mod):
    """A contiguous reward view that starts one float into its buffer: accepted by the Python layer, written by the kernel's
    dword fallback.  Same seed, same commands as an env with aligned outputs: every output bit for bit the same."""
    E = 17
    env_a, orc = _pair(amd, oracle_mod, E, seed=4300)   # (the oracle only steers the commands here)
    env_u, _ = _pair(amd, oracle_mod, E, seed=4300)
    emb_a, emb_u = _Embedded(env_a, E, lead=4), _Embedded(env_u, E, lead=1)
    assert emb_u.rew.data_ptr() % 16 == 4
    rng = np.random.default_rng(18)
    for t in range(STEPS):
        act = _commands(rng, orc, np.float32)
        orc.step(act)
        env_a.step(act, out=emb_a.out())
        env_u.step(act, out=emb_u.out())
        ctx = f"unaligned out= step {t}"
        emb_a.check_sentinels(ctx + " (aligned)")
        emb_u.check_sentinels(ctx)
        np.testing.assert_array_equal(_np(emb_u.rew).view(np.uint32), _np(emb_a.rew).view(np.uint32), err_msg=ctx + " rewards")
        np.testing.assert_array_equal(_np(emb_u.done), _np(emb_a.done), err_msg=ctx + " dones")
        np.testing.assert_array_equal(_np(emb_u.obs).view(np.uint32), _np(emb_a.obs).view(np.uint32), err_msg=ctx + " obs")
        sa, su = env_a.get_state(), env_u.get_state()
        for k in ("loc", "vel", "flags"):
            np.testing.assert_array_equal(_np(su[k]), _np(sa[k]), err_msg=f"{ctx} {k}")
    env_a.close()
    env_u.close()

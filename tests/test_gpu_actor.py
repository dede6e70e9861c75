"""FusedActor (libuavx_actor.so) on the MI355X against float64 / float32 / bf16 torch forwards of the same policy.py modules,
the exploration modes of their act(), zero-copy use of the replay ring, graph capture, snapshot semantics, checkpoints and
non-finite rows."""
import copy
import ctypes

import pytest
import torch

from fused_ref import heads as _heads
from gym_uav_collision_avoidance_amd import policy

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROWS = (1, 63, 64, 65, 4097, 262144, 524288)
ACTORS = {"sac": policy.GaussianPolicy, "td3": policy.TD3Actor, "ddpg": policy.DDPGActor}


def _fused(m, precision="f32"):
    from gym_uav_collision_avoidance_amd.fused_actor import FusedActor
    return FusedActor.from_module(m, precision=precision)


def _module(name, seed, scale):
    torch.manual_seed(seed)
    m = ACTORS[name]().to(DEV).eval()
    if scale != 1:
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(scale)
    return m


def _obs(rows, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn((rows, 10), generator=g, device=DEV)


def _raw(fa, x):
    r = fa.raw(x)
    return torch.cat(r, dim=-1) if isinstance(r, tuple) else r


@pytest.mark.parametrize("scale", [1, 3])
@pytest.mark.parametrize("name", sorted(ACTORS))
def test_fused_f32_matches_float64_reference(name, scale):
    """f32 MFMA kernel, RAW and DETERMINISTIC: max error against float64 <= max(3 x torch-f32's own error, 2e-6), and
    <= 1e-5 x max(1, largest |output|).  The second bound is 1e-5 absolute for actions and for pre-tanh outputs up to 1;
    with x3 weights the pre-tanh outputs reach 15-16, where torch-f32 itself is 8.5e-6 (SAC) / 1.14e-5 (DDPG) off.
    Measured on an MI355X: fused 3.7e-7 / 5.1e-7 (x1), 8.9e-6 / 1.31e-5 (x3 RAW), 4.0e-6 / 5.0e-6 (x3 actions)."""
    m = _module(name, 11, scale)
    fa = _fused(m)
    x = _obs(ROWS[-1])
    ref = _heads(copy.deepcopy(m).double(), x.double())
    t32 = _heads(m, x).double()
    worst = {}
    for rows in ROWS:
        for mode in ("raw", "det"):
            if mode == "raw":
                got, r, t = _raw(fa, x[:rows]).double(), ref[:rows], t32[:rows]
            else:
                got, r, t = fa.act(x[:rows]).double(), torch.tanh(ref[:rows, :2]), torch.tanh(t32[:rows, :2])
            assert got.shape == r.shape
            e_f, e_t = (got - r).abs().max().item(), (t - r).abs().max().item()
            worst[f"{mode}_{rows}"] = (e_f, e_t, r.abs().max().item())
    for key, (e_f, e_t, mag) in worst.items():
        assert e_f <= max(3 * e_t, 2e-6), (name, scale, key, e_f, e_t)
        assert e_f <= 1e-5 * max(1.0, mag), (name, scale, key, e_f, mag)


@pytest.mark.parametrize("scale", [1, 3])
@pytest.mark.parametrize("name", sorted(ACTORS))
def test_fused_bf16_accuracy(name, scale):
    """bf16 kernel (bf16 operands, f32 accumulation, bias and epilogue in f32) against float64, every row count:
    max abs error <= 7.5e-2 and <= max(5e-2, 1.25 x that of module.to(bfloat16) on bf16 observations); mean abs error
    <= 1.5 x torch-bf16's (judged from 4 097 rows up: the mean of a few dozen rows says nothing).
    Calibrated on an MI355X: worst max error 2.8e-3 (x1 weights; torch bf16 3.4e-3) and 5.8e-2 (x3 weights, SAC / TD3
    at 262 144 rows; torch bf16 5.4e-2 there, so the proposed flat 5e-2 is tighter than torch's own bf16 forward); mean
    error 0.77-0.91 x torch-bf16's."""
    m = _module(name, 12, scale)
    fa = _fused(m, "bf16")
    x = _obs(ROWS[-1], seed=2)
    ref = torch.tanh(_heads(copy.deepcopy(m).double(), x.double())[:, :2])
    tb = torch.tanh(_heads(copy.deepcopy(m).to(torch.bfloat16), x.to(torch.bfloat16))[:, :2]).double()
    res = {}
    for rows in ROWS:
        err, err_t = (fa.act(x[:rows]).double() - ref[:rows]).abs(), (tb[:rows] - ref[:rows]).abs()
        res[rows] = (err.max().item(), err_t.max().item(), err.mean().item(), err_t.mean().item())
    for rows, (mx, mx_t, m_f, m_t) in res.items():
        assert mx <= 7.5e-2 and mx <= max(5e-2, 1.25 * mx_t), (name, scale, rows, mx, mx_t)
        if rows >= 4097:
            assert m_f <= 1.5 * m_t, (name, scale, rows, m_f, m_t)


@pytest.mark.parametrize("name", sorted(ACTORS))
def test_fused_exploration_matches_module_act(name):
    m = _module(name, 13, 1)
    fa = _fused(m)
    x = _obs(4097, seed=3)
    if name == "ddpg":
        g = torch.Generator(device=DEV).manual_seed(4)
        noise = 1.5 * torch.randn((4097, 2), generator=g, device=DEV)
        ref, got = m.act(x, evaluate=False, noise=noise), fa.act(x, evaluate=False, noise=noise)
        assert ((got.abs() == 1.0).sum() > 100).item()                 # clamping reached in many rows
        sat = ref.abs() == 1.0
        assert torch.equal(got[sat], ref[sat])
        # an OU-style noise vector broadcast over rows
        n1 = torch.tensor([0.3, -2.0], device=DEV)
        torch.testing.assert_close(fa.act(x, evaluate=False, noise=n1), m.act(x, evaluate=False, noise=n1), atol=2e-6, rtol=0)
    else:
        kw = {} if name == "sac" else dict(noise_std=0.4)
        ref = m.act(x, evaluate=False, generator=torch.Generator(device=DEV).manual_seed(5), **kw)
        got = fa.act(x, evaluate=False, generator=torch.Generator(device=DEV).manual_seed(5), **kw)
        if name == "td3":
            assert ((got.abs() == 1.0).sum() > 0).item()
    torch.testing.assert_close(got, ref, atol=2e-6, rtol=0)
    assert not torch.equal(got, fa.act(x))                             # the noise did something


def test_fused_zero_copy_into_replay_slot_and_strides():
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    m = _module("sac", 14, 1)
    fa = _fused(m)
    env = BatchedMultiUAVWorld2D(128, num_agents=4, device=DEV, seed=3)
    mem = DeviceReplay(env, horizon=3)
    mem.begin(env.reset())
    mem.act.fill_(7.0)
    out = mem.action_slot()
    ptr = out.data_ptr()
    res = fa.act(mem.state, out=out)
    assert res.data_ptr() == ptr and out.data_ptr() == ptr
    assert torch.equal(out, fa.act(mem.state.clone()))
    k = mem.count % mem.L
    others = torch.cat([mem.act[i] for i in range(mem.L) if i != k])
    assert bool((others == 7.0).all())
    # obs and out as strided views inside wider rows: the neighbouring columns are not written
    rows = 1000
    wide_in = torch.full((rows, 16), float("nan"), device=DEV)
    wide_in[:, 3:13] = _obs(rows, seed=6)
    wide_out = torch.full((rows, 5), 9.0, device=DEV)
    fa.act(wide_in[:, 3:13], out=wide_out[:, 1:3])
    assert torch.equal(wide_out[:, 1:3], fa.act(wide_in[:, 3:13].contiguous()))
    assert bool((wide_out[:, 0] == 9.0).all()) and bool((wide_out[:, 3:] == 9.0).all())
    env.close()


def test_fused_graph_capture_matches_eager_ring_bitwise():
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    RING, kw = 4, dict(polar=True, auto_reset="agent0_done")
    m = _module("td3", 15, 1)
    fa = _fused(m)
    x = _obs(777, seed=7)
    a, b = fa.act(x), fa.act(x)
    assert torch.equal(a, b)
    assert torch.equal(_raw(fa, x), _raw(fa, x))
    loops = []
    for _ in range(2):
        env = BatchedMultiUAVWorld2D(256, num_agents=4, device=DEV, seed=21)
        mem = DeviceReplay(env, horizon=RING - 1)
        mem.begin(env.reset())

        def one_pass(mem=mem):
            for _ in range(RING):
                fa.act(mem.state, out=mem.action_slot())
                mem.step(**kw)
        one_pass()                          # warm (both loops alike)
        loops.append((env, mem, one_pass))
    env_e, mem_e, pass_e = loops[0]
    pass_e()
    pass_e()
    env_g, mem_g, pass_g = loops[1]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pass_g()
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for f in ("obs", "act", "rew", "done"):
        assert torch.equal(getattr(mem_e, f), getattr(mem_g, f)), f
    assert bool(mem_g.act.abs().sum() > 0)
    env_e.close()
    env_g.close()


def test_fused_snapshot_and_refresh():
    m = _module("ddpg", 16, 1)
    fa = _fused(m)
    x = _obs(300, seed=8)
    before = fa.act(x)
    with torch.no_grad():
        m.fc1.weight.mul_(-1.5)
        m.fc2.bias.add_(0.2)
    assert torch.equal(fa.act(x), before)
    fa.refresh()
    after = fa.act(x)
    assert not torch.equal(after, before)
    torch.testing.assert_close(after, m.act(x), atol=1e-5, rtol=0)


def test_fused_from_checkpoints(tmp_path):
    saves = {"sac": lambda p, m: policy.save_reference_checkpoint(str(p / "sac.chpt"), m),
             "td3": lambda p, m: policy.save_td3_checkpoint(str(p / "td3.chpt"), m),
             "ddpg": lambda p, m: policy.save_ddpg_checkpoint(str(p / "ddpg"), m)}
    x = _obs(4097, seed=9)
    for name, save in saves.items():
        m = _module(name, 17, 1)
        loaded = policy.load_actor(save(tmp_path, m), device=DEV)
        fa = _fused(loaded)
        ref = _heads(copy.deepcopy(m).double(), x.double())
        e_t = (_heads(m, x).double() - ref).abs().max().item()
        e_f = (_raw(fa, x).double() - ref).abs().max().item()
        assert e_f <= max(3 * e_t, 2e-6) and e_f <= 1e-5, (name, e_f, e_t)
        assert torch.equal(fa.act(x), _fused(m).act(x))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_fused_nonfinite_row_stays_in_its_row(precision):
    m = _module("sac", 18, 1)
    fa = _fused(m, precision)
    x = _obs(200, seed=10)
    clean = fa.act(x)
    bad = x.clone()
    bad[37, 4] = float("nan")
    bad[150, 0] = float("inf")
    got = fa.act(bad)
    assert bool(torch.isnan(got[37]).all())
    keep = torch.ones(200, dtype=torch.bool, device=DEV)
    keep[37] = keep[150] = False
    assert torch.equal(got[keep], clean[keep])


def test_fused_rejects_bad_calls():
    from gym_uav_collision_avoidance_amd import _actor_lib as A
    from gym_uav_collision_avoidance_amd.fused_actor import FusedActor
    m = _module("td3", 19, 1)
    fa = _fused(m)
    with pytest.raises(TypeError):
        fa.act(_obs(8).double())
    with pytest.raises(TypeError):
        fa.act(_obs(8).cpu())
    with pytest.raises(TypeError):
        FusedActor.from_module(torch.nn.Linear(10, 2).to(DEV))
    with pytest.raises(TypeError):
        FusedActor.from_module(copy.deepcopy(m).to(torch.bfloat16))
    with pytest.raises(ValueError):
        FusedActor.from_module(m, precision="fp8")
    lib = A.load()
    x, out = _obs(64), torch.full((64, 2), 5.0, device=DEV)
    call = lambda rows=64, ostr=10, eps=None, mode=A.DETERMINISTIC, dstr=2: lib.uavx_actor_forward(
        fa._h, x.data_ptr(), rows, ostr, eps, 0.1, mode, out.data_ptr(), dstr, None)
    assert call(rows=-1) == A.ERR_INVALID_ARG
    assert call(ostr=9) == A.ERR_INVALID_ARG
    assert call(dstr=1) == A.ERR_INVALID_ARG
    assert call(mode=4) == A.ERR_INVALID_ARG
    assert call(mode=A.ADD_CLAMP) == A.ERR_INVALID_ARG           # no eps
    assert call(mode=A.SAC_SAMPLE, eps=x.data_ptr()) == A.ERR_INVALID_ARG   # not a SAC actor
    assert call(rows=0) == A.OK
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    h = ctypes.c_void_p()
    assert lib.uavx_actor_create(A.TD3, A.F32, 10, 256, 256, 2, ctypes.byref(h)) == A.OK
    assert lib.uavx_actor_forward(h, x.data_ptr(), 64, 10, None, 0.0, A.DETERMINISTIC, out.data_ptr(), 2, None) == A.ERR_NOT_PACKED
    assert lib.uavx_actor_destroy(h) == A.OK

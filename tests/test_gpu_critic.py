"""FusedCritic / FusedTarget (libuavx_actor.so, include/uavx_critic.h) on the MI355X against float64 / float32 torch
evaluations of the policy.py critics and of the learners' own target expressions (sac.py:56-60, td3.py:114-127,
ddpg.py:62), on batches drawn from a real DeviceReplay; numerics at tanh saturation, determinism, strided inputs, graph
capture, snapshot semantics, checkpoints, one SAC critic update and argument checks."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

from fused_ref import q_module as _q_module, target_torch as _target_torch
from gym_uav_collision_avoidance_amd import _actor_lib, policy

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROWS = (1, 63, 64, 65, 255, 256, 257, 4097, 65536, 262144)
CRITICS = {"sac": policy.TwinQ, "td3": policy.TD3TwinQ, "ddpg": policy.DDPGCritic}
ACTORS = {"sac": policy.GaussianPolicy, "td3": policy.TD3Actor, "ddpg": policy.DDPGActor}


def _scaled(m, scale):
    if scale != 1:
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(scale)
    return m.to(DEV).eval()


def _pair(name, seed, scale=1):
    torch.manual_seed(seed)
    return _scaled(ACTORS[name](), scale), _scaled(CRITICS[name](), scale)


def _fc(c, precision="f32"):
    from gym_uav_collision_avoidance_amd.fused_critic import FusedCritic
    return FusedCritic.from_module(c, precision=precision)


def _ft(a, c, precision="f32", **kw):
    from gym_uav_collision_avoidance_amd.fused_critic import FusedTarget
    return FusedTarget(a, c, precision=precision, **kw)


_REPLAY = {}


def _replay_batch(rows, seed=0):
    """(next_state [B, 10], reward [B], mask [B]) sampled from a DeviceReplay after 160 fused steps of random policy
    actions with auto-reset, so that masks of 0 occur; one ring shared by the whole module."""
    if "mem" not in _REPLAY:
        from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
        from gym_uav_collision_avoidance_amd.replay import DeviceReplay
        env = BatchedMultiUAVWorld2D(1024, num_agents=4, device=DEV, seed=31)
        mem = DeviceReplay(env, horizon=160)
        mem.begin(env.reset())
        g = torch.Generator(device=DEV).manual_seed(5)
        for _ in range(160):
            mem.action_slot().copy_(torch.rand((1024, 4, 2), generator=g, device=DEV) * 2 - 1)
            mem.step(polar=True, auto_reset="agent0_done", step_cap=60)
        _REPLAY.update(env=env, mem=mem)
    g = torch.Generator(device=DEV).manual_seed(100 + seed)
    _, _, r, s2, m = _REPLAY["mem"].sample(rows, generator=g)
    return s2.contiguous(), r.contiguous(), m.contiguous()


def _eps(rows, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn((rows, 2), generator=g, device=DEV)


@pytest.mark.parametrize("scale", [1, 3])
@pytest.mark.parametrize("name", sorted(CRITICS))
def test_q_f32_matches_float64(name, scale):
    """f32 critic_q, both variants (below / above the small-batch threshold, and each forced over every row count): max
    error against float64 <= max(3 x torch-f32's own error, 2e-6) and <= 1e-5 x max(1, max|Q|).
    Measured on an MI355X at 262 144 rows (fused / torch-f32): large-batch 3.9e-7-6.5e-7 / 2.3e-7-6.3e-7 (x1),
    4.8e-6-2.3e-5 / 4.6e-6-2.3e-5 (x3, |Q| up to 29); small-batch 1.4e-7-3.2e-7 (x1), 4.1e-6-8.2e-6 (x3)."""
    _, c = _pair(name, 21, scale)
    fc = _fc(c)
    n = ROWS[-1]
    g = torch.Generator(device=DEV).manual_seed(4)
    s = torch.randn((n, 10), generator=g, device=DEV)
    a = torch.rand((n, 2), generator=g, device=DEV) * 2 - 1
    ref = _q_module(copy.deepcopy(c).double(), s.double(), a.double())
    t32 = _q_module(c, s, a).double()
    for split in (_actor_lib.SPLIT_ROWS, 0, 1 << 62):
        fc.set_split_rows(split)
        for rows in ROWS:
            q = fc.q(s[:rows], a[:rows])
            got = (torch.cat(q, dim=-1) if isinstance(q, tuple) else q).double()
            assert got.shape == ref[:rows].shape
            e_f, e_t = (got - ref[:rows]).abs().max().item(), (t32[:rows] - ref[:rows]).abs().max().item()
            mag = ref[:rows].abs().max().item()
            assert e_f <= max(3 * e_t, 2e-6), (name, scale, split, rows, e_f, e_t)
            assert e_f <= 1e-5 * max(1.0, mag), (name, scale, split, rows, e_f, mag)


@pytest.mark.parametrize("scale", [1, 3])
@pytest.mark.parametrize("name", sorted(CRITICS))
def test_q_bf16_accuracy(name, scale):
    """bf16 critic_q against float64 with test_gpu_actor.py's bf16 bounds, scaled to |Q|: max error <= max(5e-2 x
    max(1, max|Q|), 1.25 x that of module.to(bfloat16)) and mean error <= 1.5 x torch-bf16's from 4 097 rows up.
    Measured on an MI355X at 262 144 rows: 1.9e-3-5.0e-3 (x1, |Q| <= 1.1) and 5.7e-2-1.4e-1 (x3, |Q| 13-29)."""
    _, c = _pair(name, 22, scale)
    fc = _fc(c, "bf16")
    n = ROWS[-1]
    g = torch.Generator(device=DEV).manual_seed(5)
    s = torch.randn((n, 10), generator=g, device=DEV)
    a = torch.rand((n, 2), generator=g, device=DEV) * 2 - 1
    ref = _q_module(copy.deepcopy(c).double(), s.double(), a.double())
    tb = _q_module(copy.deepcopy(c).to(torch.bfloat16), s.to(torch.bfloat16), a.to(torch.bfloat16)).double()
    for rows in ROWS:
        q = fc.q(s[:rows], a[:rows])
        got = (torch.cat(q, dim=-1) if isinstance(q, tuple) else q).double()
        err, err_t = (got - ref[:rows]).abs(), (tb[:rows] - ref[:rows]).abs()
        mag = max(1.0, ref[:rows].abs().max().item())
        assert err.max().item() <= max(5e-2 * mag, 1.25 * err_t.max().item()), (name, scale, rows, err.max().item())
        if rows >= 4097:
            assert err.mean().item() <= 1.5 * err_t.mean().item(), (name, scale, rows, err.mean().item(), err_t.mean().item())


@pytest.mark.parametrize("scale", [1, 3])
@pytest.mark.parametrize("name,alpha", [("ddpg", 0.2), ("sac", 0.2), ("sac", 2.0), ("td3", 0.2)])
def test_target_f32_matches_float64(name, alpha, scale):
    """f32 critic_target against the learner's expression in float64 with the same ε, α as a device tensor, γ 0.99, on
    replay batches; aux checks a', logπ and min Q on their own.  Each quantity: max error <= max(3 x torch-f32's own
    error, 2e-6 x max(1, max|ref|)) and <= 1e-5 x max(1, max|ref|).  SAC's logπ and y are the exception to the flat bound:
    log(1 - tanh(x_t)^2 + 1e-6) is ill-conditioned in f32 near saturation, and torch-f32 itself is 4.3e-4 (x1 weights) /
    9.3e-2 (x3) off in logπ; there they must stay within 1.1 x torch-f32's error + 1e-5 x max(1, max|ref|).
    Measured on an MI355X at 262 144 rows (fused / torch-f32 error): SAC y and logπ 1.00x in both variants; a', min Q
    0.87-1.05x; TD3 / DDPG every quantity 0.54-1.05x (x1: <= 2.6e-7; x3: <= 4.2e-6)."""
    act, c = _pair(name, 23, scale)
    ft = _ft(act, c)
    n = ROWS[-1]
    s2, r, m = _replay_batch(n)
    assert bool((m == 0).any()) and bool((m == 1).any())
    eps = _eps(n)
    al = torch.tensor([alpha], device=DEV)
    ref = _target_torch(name, act, c, s2, r, m, eps, alpha)
    t32 = [t.double() for t in _target_torch(name, act, c, s2, r, m, eps, alpha, dtype=torch.float32)]
    for rows in ROWS:
        aux = torch.empty((rows, 4), device=DEV)
        y = ft(s2[:rows], r[:rows], m[:rows], alpha=al, noise=eps[:rows].contiguous(), aux=aux)
        assert y.shape == (rows, 1) and y.dtype == torch.float32
        got = (y, aux[:, 0:2], aux[:, 2:3], aux[:, 3:4])
        for what, gv, rv, tv in zip(("y", "a", "logpi", "minq"), got, ref, t32):
            gv, rv, tv = gv.double(), rv[:rows], tv[:rows]
            e_f, e_t = (gv - rv).abs().max().item(), (tv - rv).abs().max().item()
            mag = max(1.0, rv.abs().max().item())
            assert e_f <= max(3 * e_t, 2e-6 * mag), (name, scale, alpha, rows, what, e_f, e_t)
            if name == "sac" and what in ("y", "logpi"):
                assert e_f <= 1.1 * e_t + 1e-5 * mag, (name, scale, alpha, rows, what, e_f, e_t)
            else:
                assert e_f <= 1e-5 * mag, (name, scale, alpha, rows, what, e_f, mag)


@pytest.mark.parametrize("name", sorted(CRITICS))
def test_target_bf16_tracks_torch_bf16(name):
    """bf16 critic_target (a' rounded to bf16 before the critic) against float64: max error <= max(5e-2 x max(1, |y|),
    1.25 x that of the block run with bf16 modules)."""
    act, c = _pair(name, 24)
    ft = _ft(act, c, "bf16")
    s2, r, m = _replay_batch(65536, seed=1)
    eps = _eps(65536)
    ref = _target_torch(name, act, c, s2, r, m, eps, 0.2)[0]
    tb = _target_torch(name, act, c, s2, r, m, eps, 0.2, dtype=torch.bfloat16)[0].double()
    y = ft(s2, r, m, alpha=0.2, noise=eps).double()
    err, err_t = (y - ref).abs().max().item(), (tb - ref).abs().max().item()
    assert err <= max(5e-2 * max(1.0, ref.abs().max().item()), 1.25 * err_t), (name, err, err_t)


def test_sac_saturation_gives_torch_log_correction():
    """|x_t| >= 10, where tanhf is ±1 in f32: the correction is torch-f32's log(1e-6), not a saturation-free form."""
    act, c = _pair("sac", 25)
    ft = _ft(act, c)
    s2, r, m = _replay_batch(1000, seed=2)
    eps = _eps(1000, seed=9) * 40.0
    eps[:, 0] = eps[:, 0].sign() * eps[:, 0].abs().clamp(min=30.0)
    aux = torch.empty((1000, 4), device=DEV)
    ft(s2, r, m, alpha=0.2, noise=eps, aux=aux)
    _, a32, lp32, _ = _target_torch("sac", act, c, s2, r, m, eps, 0.2, dtype=torch.float32)
    with torch.no_grad():
        mean, log_std = act(s2)
        x_t = mean + eps * log_std.exp()
    assert bool((x_t[:, 0].abs() >= 10).all())
    assert bool((aux[:, 0].abs() == 1.0).all()) and torch.equal(aux[:, 0], a32[:, 0])
    torch.testing.assert_close(aux[:, 1], a32[:, 1], rtol=0, atol=1e-5)
    assert bool(torch.isfinite(aux[:, 2]).all())
    # the saturated dimension contributes -log(1e-6) = +13.8 on top of the Gaussian term, as in torch-f32
    torch.testing.assert_close(aux[:, 2:3], lp32, rtol=1e-5, atol=1e-4)


def test_determinism_nan_row_and_variants():
    act, c = _pair("td3", 26)
    ft = _ft(act, c)
    s2, r, m = _replay_batch(40000, seed=3)
    eps = _eps(40000)
    for split in (_actor_lib.SPLIT_ROWS, 0):
        ft.set_split_rows(split)
        y1, y2 = ft(s2, r, m, noise=eps), ft(s2, r, m, noise=eps)
        assert torch.equal(y1, y2)
    # within one variant a row's result does not depend on the batch size
    ft.set_split_rows(1 << 62)
    small = [ft(s2[:n], r[:n], m[:n], noise=eps[:n].contiguous()) for n in (63, 257, 20000)]
    assert torch.equal(small[0], small[1][:63]) and torch.equal(small[1], small[2][:257])
    ft.set_split_rows(0)
    large = [ft(s2[:n], r[:n], m[:n], noise=eps[:n].contiguous()) for n in (63, 257, 20000)]
    assert torch.equal(large[0], large[1][:63]) and torch.equal(large[1], large[2][:257])
    # across the switch: the same to f32 rounding
    torch.testing.assert_close(small[2], large[2], rtol=1e-5, atol=1e-5)
    # a NaN row stays in its row
    for split in (1 << 62, 0):
        ft.set_split_rows(split)
        bad = s2[:300].clone()
        bad[37, 4] = float("nan")
        y = ft(bad, r[:300], m[:300], noise=eps[:300].contiguous())
        ok = ft(s2[:300], r[:300], m[:300], noise=eps[:300].contiguous())
        assert bool(torch.isnan(y[37]).all())
        keep = torch.ones(300, dtype=torch.bool, device=DEV)
        keep[37] = False
        assert torch.equal(y[keep], ok[keep])


def test_strided_inputs_and_outputs():
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    act, c = _pair("sac", 27)
    ft = _ft(act, c)
    env = BatchedMultiUAVWorld2D(256, num_agents=4, device=DEV, seed=3)
    mem = DeviceReplay(env, horizon=3)
    mem.begin(env.reset())
    for _ in range(2):
        mem.action_slot().uniform_(-1, 1)
        mem.step(polar=True)
    view = mem.obs[1, :, 1]                                    # [256, 10] view of the ring, row stride 40
    assert view.stride(0) == 40
    rews = mem.rew[0, :, 1]                                    # [256], stride 4
    masks = 1.0 - mem.done[0, :, 1].float()
    eps = _eps(256)
    ref = ft(view.contiguous(), rews.contiguous(), masks.contiguous(), alpha=0.2, noise=eps)
    assert torch.equal(ft(view, rews, masks, alpha=0.2, noise=eps), ref)
    assert torch.equal(ft(view, rews.unsqueeze(1), masks.reshape(-1, 1), alpha=0.2, noise=eps), ref)
    wide = torch.full((256, 3), 9.0, device=DEV)
    ft(view, rews, masks, alpha=0.2, noise=eps, out=wide[:, 1])
    assert torch.equal(wide[:, 1:2], ref) and bool((wide[:, 0] == 9.0).all()) and bool((wide[:, 2] == 9.0).all())
    fc = _fc(c)
    acts = mem.act[1, :, 1]
    q1, q2 = fc.q(view, acts)
    r1, r2 = fc.q(view.contiguous(), acts.contiguous())
    assert torch.equal(q1, r1) and torch.equal(q2, r2)
    env.close()


def test_graph_capture_sample_refresh_target_matches_eager():
    act, c = _pair("sac", 28)
    ft = _ft(act, c)
    _replay_batch(1)
    mem = _REPLAY["mem"]
    alpha = torch.tensor([0.2], device=DEV)
    out = torch.empty((256, 1), device=DEV)

    def block(gen):
        _, _, r, s2, m = mem.sample(256, generator=gen)
        ft.refresh()
        ft(s2, r, m, alpha=alpha, generator=gen, out=out)
        return out

    ge = torch.Generator(device=DEV).manual_seed(77)
    eager = block(ge).clone()
    gg = torch.Generator(device=DEV).manual_seed(77)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    graph.register_generator_state(gg)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        block(torch.Generator(device=DEV).manual_seed(1))    # warm on the side stream
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(graph):
        block(gg)
    gg.manual_seed(77)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    # the graph reads alpha when it runs
    alpha.fill_(2.0)
    gg.manual_seed(77)
    graph.replay()
    torch.cuda.synchronize()
    ge.manual_seed(77)
    assert torch.equal(out.clone(), block(ge))
    assert not torch.equal(out, eager)


def test_refresh_semantics_after_soft_update():
    act, c = _pair("td3", 29)
    tgt_c = copy.deepcopy(c)
    ft = _ft(act, tgt_c)
    s2, r, m = _replay_batch(4097, seed=4)
    eps = _eps(4097)
    before = ft(s2, r, m, noise=eps).clone()
    torch.manual_seed(1)
    live = CRITICS["td3"]().to(DEV)
    with torch.no_grad():                                      # td3.py soft update, tau 0.005
        for p, tp in zip(live.parameters(), tgt_c.parameters()):
            tp.mul_(1 - 0.005).add_(0.005 * p)
    assert torch.equal(ft(s2, r, m, noise=eps), before)
    ft.refresh()
    after = ft(s2, r, m, noise=eps)
    assert not torch.equal(after, before)
    ref = _target_torch("td3", act, tgt_c, s2, r, m, eps, 0.2)[0]
    assert (after.double() - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())


def test_construction_from_reference_checkpoints(tmp_path):
    from gym_uav_collision_avoidance_amd.fused_critic import FusedTarget
    s2, r, m = _replay_batch(1000, seed=5)
    eps = _eps(1000)
    torch.manual_seed(30)
    paths = {"sac": policy.save_reference_checkpoint(str(tmp_path / "sac.chpt"), policy.GaussianPolicy()),
             "td3": policy.save_td3_checkpoint(str(tmp_path / "td3.chpt"), policy.TD3Actor()),
             "ddpg": policy.save_ddpg_checkpoint(str(tmp_path / "ddpg"), policy.DDPGActor())}
    for name, p in paths.items():
        a, c = policy.load_target_networks(p, device=DEV)
        assert isinstance(a, ACTORS[name]) and isinstance(c, CRITICS[name])
        ft = FusedTarget(a, c)
        assert ft.learner == name
        y = ft(s2, r, m, alpha=0.2, noise=eps)
        ref = _target_torch(name, a, c, s2, r, m, eps, 0.2)[0]
        assert (y.double() - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item()), name


def test_sac_critic_update_with_fused_target():
    """sac.py:61-68 with next_q_value from FusedTarget: both losses agree with the torch block's to 1e-5 relative."""
    act, c = _pair("sac", 31)
    crit = copy.deepcopy(c)
    ft = _ft(act, c)
    s, a = torch.randn((256, 10), device=DEV), torch.rand((256, 2), device=DEV) * 2 - 1
    s2, r, m = _replay_batch(256, seed=6)
    eps = _eps(256)
    nq_f = ft(s2, r, m, alpha=0.2, noise=eps)
    nq_t = _target_torch("sac", act, c, s2, r, m, eps, 0.2, dtype=torch.float32)[0]
    qf1, qf2 = crit(s, a)
    for nq in (nq_f, nq_t):
        assert nq.shape == qf1.shape
    l_f = (F.mse_loss(qf1, nq_f).item(), F.mse_loss(qf2, nq_f).item())
    l_t = (F.mse_loss(qf1, nq_t).item(), F.mse_loss(qf2, nq_t).item())
    for x, y in zip(l_f, l_t):
        assert abs(x - y) <= 1e-5 * max(1.0, abs(y)), (l_f, l_t)
    loss = F.mse_loss(qf1, nq_f) + F.mse_loss(qf2, nq_f)
    loss.backward()                                            # the fused target is a plain (graph-free) tensor
    assert crit.linear1.weight.grad is not None and not nq_f.requires_grad


def test_bad_calls_raise():
    from gym_uav_collision_avoidance_amd.fused_critic import FusedCritic, FusedTarget
    act, c = _pair("sac", 32)
    ft = _ft(act, c)
    s2, r, m = _replay_batch(64, seed=7)
    with pytest.raises(TypeError):
        ft(s2.cpu(), r, m, alpha=0.2)
    with pytest.raises(TypeError):
        ft(s2.double(), r, m, alpha=0.2)
    with pytest.raises(ValueError):
        ft(s2[:, :9], r, m, alpha=0.2)
    with pytest.raises(ValueError):
        ft(s2, r[:10], m, alpha=0.2)
    with pytest.raises(ValueError):
        ft(s2, r, m)                                           # SAC without alpha
    with pytest.raises(TypeError):
        ft(s2, r, m, alpha=torch.tensor([0.2], dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError):
        _ft(policy.TD3Actor().to(DEV), c)                      # mismatched pair
    with pytest.raises(TypeError):
        FusedCritic.from_module(copy.deepcopy(c).double())
    with pytest.raises(ValueError):
        FusedTarget(_ft(act, c).actor, _fc(c, "bf16"))        # mismatched precision
    fc = _fc(c)
    with pytest.raises(ValueError):
        fc.q(s2, torch.zeros((63, 2), device=DEV))
    # the C ABI with live handles: mismatched kind / precision, NULL buffers, negative rows, SAC without alpha
    lib = _actor_lib.load()
    td3a = _ft(*_pair("td3", 33)).actor
    bf_a = _ft(act, c, "bf16").actor
    buf = ctypes.c_void_p(s2.data_ptr())
    al = ctypes.c_void_p(r.data_ptr())
    call = lambda actor, rows=4, ns=buf, alpha=al: lib.uavx_critic_target(
        fc._h, actor._h, ns, rows, 10, buf, 1, buf, 1, buf, alpha, 0.99, 0.2, 0.5, buf, 1, None, 4, None)
    assert call(td3a) == _actor_lib.ERR_INVALID_ARG
    assert call(bf_a) == _actor_lib.ERR_INVALID_ARG
    assert call(ft.actor, ns=None) == _actor_lib.ERR_INVALID_ARG
    assert call(ft.actor, rows=-1) == _actor_lib.ERR_INVALID_ARG
    assert call(ft.actor, alpha=None) == _actor_lib.ERR_INVALID_ARG
    assert lib.uavx_critic_q(fc._h, buf, -1, 10, buf, 2, buf, 2, None) == _actor_lib.ERR_INVALID_ARG
    assert lib.uavx_critic_q(fc._h, None, 4, 10, buf, 2, buf, 2, None) == _actor_lib.ERR_INVALID_ARG
    assert lib.uavx_critic_q(fc._h, buf, 4, 10, buf, 2, buf, 1, None) == _actor_lib.ERR_INVALID_ARG   # twin: 2 columns
    assert lib.uavx_critic_pack(fc._h, *([buf] * 6), *([None] * 6), None) == _actor_lib.ERR_INVALID_ARG  # second tower
    torch.cuda.synchronize()

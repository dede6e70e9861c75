"""FusedActionGrad and FusedActorLoss (libuavx_actor.so, include/uavx_action_grad.h) on the MI355X against float64 and
float32 torch autograd (tests/action_grad_ref.py): accuracy away from activation kinks, the kinks themselves, every hidden
size, the tower mask, ragged rows and strides over NaN memory, determinism and row independence, live weights, the autograd
function, the three learners' actor-loss blocks, graph capture and argument checks."""
import copy
import ctypes

import pytest
import torch

from action_grad_ref import actor, actor_grads, actor_preacts, analytic, jacobian, sac_sample
from grad_ref import critic, preacts, towers
from gym_uav_collision_avoidance_amd import _actor_lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROWS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4097)
NAN = float("nan")


def _ag(m):
    from gym_uav_collision_avoidance_amd.fused_critic import FusedActionGrad
    return FusedActionGrad(m)


def _away(z, margin):
    return (z.abs() >= margin * z.pow(2).mean().sqrt()).all(1)


def _batch(m, rows, seed, margin=1e-4):
    """rows of (s, a) whose every float64 pre-activation of every tower is at least margin x its layer's RMS away from 0."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = 3 * rows + 256
    s = torch.randn((n, 10), generator=g, device=DEV)
    a = torch.rand((n, 2), generator=g, device=DEV) * 2 - 1
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    for z1, z2 in preacts(m, s, a):
        keep &= _away(z1, margin) & _away(z2, margin)
    idx = keep.nonzero().squeeze(1)[:rows]
    assert idx.numel() == rows
    return s[idx].contiguous(), a[idx].contiguous()


def _fused(m, s, a, towers=None, out=None):
    q, j = _ag(m).q_dqda(s, a, towers=towers, out=out)
    torch.cuda.synchronize()
    return q, j


def _within(f, r64, t32, what):
    """max-abs error of f against float64 <= max(2 x torch-f32's own, 2e-6 max|reference|)."""
    ef = float((f.double() - r64).abs().max())
    et = float((t32.double() - r64).abs().max())
    top = float(r64.abs().max())
    print(f"{what}: fused {ef:.3e} torch-f32 {et:.3e} max|ref| {top:.3e}")
    assert ef <= max(2 * et, 2e-6 * top), f"{what}: fused {ef:.3e} torch-f32 {et:.3e} max|ref| {top:.3e}"


def _check(m, s, a, what):
    q, j = _fused(m, s, a)
    q64, j64 = jacobian(m, s, a, torch.float64)
    q32, j32 = jacobian(m, s, a, torch.float32)
    assert q.shape == (len(q64), s.shape[0]) and j.shape == (len(q64), s.shape[0], 2)
    for t in range(len(q64)):
        _within(q[t], q64[t], q32[t], f"{what} q{t + 1}")
        _within(j[t], j64[t], j32[t], f"{what} J{t + 1}")


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_accuracy_against_float64(kind):
    """Measured on the MI355X, over this test and test_every_hidden_size: the fused q is at most 3.8e-7 and the fused J at
    most 5.6e-7 of the tensor maximum from float64 (torch-f32: 2.0e-6 and 7.8e-7); the largest error / bound ratio is 0.19
    for q and 0.28 for J."""
    m = critic(kind, 11, device=DEV)
    for rows in ROWS:
        s, a = _batch(m, rows, seed=rows)
        _check(m, s, a, f"{kind}/{rows}")


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_kinks_follow_torch(kind):
    """s = a = 0 and every layer-1 bias 0 give z1 = 0 exactly; half the layer-2 biases 0 give z2 = 0 there too.  relu'(0) = 0
    and leaky'(0) = 0.01 as torch: q and J match torch-f32's, and a slope of 1 at 0 would not."""
    m = critic(kind, 12, device=DEV)
    with torch.no_grad():
        for t in towers(m):
            t[1].zero_()
            t[3][::2] = 0.0
    s, a = torch.zeros((16, 10), device=DEV), torch.zeros((16, 2), device=DEV)
    q, j = _fused(m, s, a)
    q32, j32 = jacobian(m, s, a, torch.float32)
    _, jk = analytic(m, s, a, kink_slope=1.0)
    flip = 0.0
    for t in range(len(q32)):
        assert float((q[t] - q32[t]).abs().max()) <= 1e-5 * float(q32[t].abs().max())
        scale = float(j32[t].abs().max()) + 1e-30
        assert float((j[t] - j32[t]).abs().max()) <= 1e-5 * scale, float((j[t] - j32[t]).abs().max()) / scale
        flip = max(flip, float((jk[t].float() - j32[t]).abs().max()) / scale)
    assert flip > 1e-3, flip


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_every_hidden_size(kind):
    """Partial layer-1 blocks, a single layer-2 block, fewer unit blocks than waves, and the widest layer 2."""
    h1s = (385, 393, 400) if kind == "ddpg" else (241, 248, 256)
    for h1 in h1s:
        for h2 in (1, 15, 16, 17, 31, 33, 100, 255, 300):
            m = critic(kind, h1 + h2, hidden1=h1, hidden2=h2, device=DEV)
            for rows in (17, 257):
                s, a = _batch(m, rows, seed=h2 + rows)
                _check(m, s, a, f"{kind} {h1}x{h2} rows {rows}")
    m = critic(kind, 4096, hidden1=h1s[-1], hidden2=4096, device=DEV)
    s, a = _batch(m, 17, seed=4096)
    _check(m, s, a, f"{kind} {h1s[-1]}x4096 rows 17")


def test_tower_mask():
    for kind in ("sac", "td3"):
        m = critic(kind, 13, device=DEV)
        s, a = _batch(m, 257, seed=3)
        both = _fused(m, s, a, towers=3)
        for mask in (1, 2, 3):
            q = torch.full((2, 257), NAN, device=DEV)
            j = torch.full((2, 257, 2), NAN, device=DEV)
            rq, rj = _fused(m, s, a, towers=mask, out=(q, j))
            assert rq is q and rj is j
            for t in range(2):
                if mask >> t & 1:
                    assert torch.equal(q[t], both[0][t]) and torch.equal(j[t], both[1][t])
                    assert bool(torch.isfinite(q[t]).all()) and bool(torch.isfinite(j[t]).all())
                else:
                    assert bool(torch.isnan(q[t]).all()) and bool(torch.isnan(j[t]).all())
    m = critic("ddpg", 13, device=DEV)
    s, a = _batch(m, 17, seed=3)
    assert all(torch.equal(x, r) for x, r in zip(_fused(m, s, a, towers=1), _fused(m, s, a)))


def test_ragged_rows_and_strides_over_nan_memory():
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    env = BatchedMultiUAVWorld2D(256, num_agents=4, device=DEV, seed=3)
    mem = DeviceReplay(env, horizon=8)
    mem.begin(env.reset())
    for _ in range(4):
        mem.action_slot().uniform_(-1, 1)
        mem.step(polar=True)
    G = 64
    for kind in ("sac", "ddpg"):
        m = critic(kind, 14, device=DEV)
        T = len(towers(m))
        for rows in (1, 17, 255):
            s, a = _batch(m, rows, seed=7)
            ref = _fused(m, s.clone(), a.clone())
            assert all(bool(torch.isfinite(x).all()) for x in ref)
            # the last `rows` rows of NaN-filled allocations, outputs between NaN guards
            big_s = torch.full((rows + 40, 10), NAN, device=DEV)
            big_a = torch.full((rows + 40, 2), NAN, device=DEV)
            big_s[-rows:], big_a[-rows:] = s, a
            fq = torch.full((2 * G + T * rows,), NAN, device=DEV)
            fj = torch.full((2 * G + T * rows * 2,), NAN, device=DEV)
            out = (fq[G:G + T * rows].view(T, rows), fj[G:G + T * rows * 2].view(T, rows, 2))
            got = _fused(m, big_s[-rows:], big_a[-rows:], out=out)
            assert all(torch.equal(x, r) for x, r in zip(got, ref))
            for f in (fq, fj):
                assert bool(torch.isnan(f[:G]).all()) and bool(torch.isnan(f[-G:]).all())
            # [:, :10] / [:, :2] of wider NaN-filled tensors
            wide_s = torch.full((rows, 13), NAN, device=DEV)
            wide_a = torch.full((rows, 7), NAN, device=DEV)
            wide_s[:, :10], wide_a[:, :2] = s, a
            got = _fused(m, wide_s[:, :10], wide_a[:, :2])
            assert all(torch.equal(x, r) for x, r in zip(got, ref))
            # views of the replay ring: [rows, 10] stride 40, [rows, 2] stride 8
            s_view, a_view = mem.obs[2, :rows, 1], mem.act[2, :rows, 1]
            if rows > 1:
                assert s_view.stride(0) == 40 and a_view.stride(0) == 8
            got = _fused(m, s_view, a_view)
            assert all(torch.equal(x, r) for x, r in zip(got, _fused(m, s_view.contiguous(), a_view.contiguous())))
    env.close()


def test_determinism_and_row_independence():
    for kind in ("sac", "td3", "ddpg"):
        m = critic(kind, 15, device=DEV)
        s, a = _batch(m, 257, seed=5)
        ag = _ag(m)
        q1, j1 = ag.q_dqda(s, a)
        q2, j2 = ag.q_dqda(s, a)
        assert torch.equal(q1, q2) and torch.equal(j1, j2)
        # one variant for every row count: a row's results do not depend on the batch around it
        q16, j16 = ag.q_dqda(s[:16], a[:16])
        assert torch.equal(q16, q1[:, :16]) and torch.equal(j16, j1[:, :16])
        q17, j17 = ag.q_dqda(s[240:257], a[240:257])
        assert torch.equal(q17, q1[:, 240:]) and torch.equal(j17, j1[:, 240:])
        # a NaN input row gives NaN in its own row only
        sn, an = s.clone(), a.clone()
        sn[5, 3] = NAN
        an[40, 1] = NAN
        qn, jn = ag.q_dqda(sn, an)
        ok = torch.ones(257, dtype=torch.bool, device=DEV)
        ok[5] = ok[40] = False
        assert bool(torch.isnan(qn[:, ~ok]).all())
        assert torch.equal(qn[:, ok], q1[:, ok]) and torch.equal(jn[:, ok], j1[:, ok])


def test_live_weights_and_untouched_snapshot():
    from gym_uav_collision_avoidance_amd.fused_critic import FusedCritic
    m = critic("td3", 16, device=DEV)
    s0, a0 = _batch(m, 256, seed=1)
    fc = FusedCritic.from_module(m)
    snap = [q.clone() for q in fc.q(s0, a0)]
    ag = _ag(fc)
    q0, j0 = (x.clone() for x in ag.q_dqda(s0, a0))
    g = torch.Generator(device=DEV).manual_seed(2)
    with torch.no_grad():
        for p in m.parameters():                       # what an optimiser step does: in place, no refresh()
            p.add_(torch.randn(p.shape, generator=g, device=DEV) * 0.01)
    s, a = _batch(m, 256, seed=1)                      # the new weights move the kinks
    q1, j1 = ag.q_dqda(s, a)
    q64, j64 = jacobian(m, s, a, torch.float64)
    q32, j32 = jacobian(m, s, a, torch.float32)
    for t in range(2):
        _within(q1[t], q64[t], q32[t], f"live q{t + 1}")
        _within(j1[t], j64[t], j32[t], f"live J{t + 1}")
    assert not torch.equal(j1, j0)
    # the FusedCritic snapshot is neither read nor changed
    assert all(torch.equal(q, r) for q, r in zip(fc.q(s0, a0), snap))
    fc.refresh()
    assert not torch.equal(fc.q(s0, a0)[0], snap[0])


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_autograd_function(kind):
    m = critic(kind, 17, device=DEV)
    s, a = _batch(m, 257, seed=9)
    if kind != "ddpg":                                 # and away from the tie of torch.min
        with torch.no_grad():
            d = torch.sub(*copy.deepcopy(m).double()(s.double(), a.double())).squeeze(1)
        keep = d.abs() >= 1e-4 * d.pow(2).mean().sqrt()
        s, a = s[keep].contiguous(), a[keep].contiguous()
        assert s.shape[0] >= 200
    ag = _ag(m)
    c1, c2 = 0.7, -1.3

    def losses(out):
        qs = list(out) if isinstance(out, tuple) else [out]
        ls = [sum(c * q for c, q in zip((c1, c2), qs)).sum()]
        return ls + ([torch.min(*qs).sum()] if len(qs) == 2 else [])

    def grads(fn, dtype):
        ss = s.detach().clone().to(dtype).requires_grad_(True)
        aa = a.detach().clone().to(dtype).requires_grad_(True)
        out = []
        for i in range(1 if kind == "ddpg" else 2):
            aa.grad = None
            losses(fn(ss, aa))[i].backward()
            out.append(aa.grad.clone())
        return out, ss

    gf, ss = grads(ag, torch.float32)
    assert ss.grad is None and all(p.grad is None for p in m.parameters())
    g32, _ = grads(copy.deepcopy(m), torch.float32)
    g64, _ = grads(copy.deepcopy(m).double(), torch.float64)
    for i, (f, r, t) in enumerate(zip(gf, g64, g32)):
        _within(f, r, t, f"{kind} d loss{i} / da")
    out = ag(s, a)                                     # what the module's forward returns
    ref = m(s, a)
    for x, r in zip(out if isinstance(out, tuple) else (out,), ref if isinstance(ref, tuple) else (ref,)):
        assert x.shape == r.shape == (s.shape[0], 1)
    if kind != "ddpg":
        q1 = ag(s, a, towers=1)
        assert torch.is_tensor(q1) and torch.equal(q1, out[0])


def _actor_batch(kind, pol, crit, rows, seed, margin=1e-4):
    """States (and SAC's eps) kept when, in float64: the actor's pre-activations, the critic's at a = pi(s) and q1 − q2 are
    margin x RMS away from 0, and the raw log-std is margin away from both clamps."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = 3 * rows + 256
    s = torch.randn((n, 10), generator=g, device=DEV)
    eps = torch.randn((n, 2), generator=g, device=DEV) if kind == "sac" else None
    (z1, z2), raw = actor_preacts(kind, pol, s)
    keep = _away(z1, margin) & _away(z2, margin)
    p64 = copy.deepcopy(pol).double()
    with torch.no_grad():
        if kind == "sac":
            keep &= ((raw - 2).abs() >= margin).all(1) & ((raw + 20).abs() >= margin).all(1)
            a = sac_sample(p64, s.double(), eps.double())[0]
        else:
            a = p64(s.double())
        for c1, c2 in preacts(crit, s.double(), a):
            keep &= _away(c1, margin) & _away(c2, margin)
        if kind != "ddpg":
            d = torch.sub(*copy.deepcopy(crit).double()(s.double(), a)).squeeze(1)
            keep &= d.abs() >= margin * d.pow(2).mean().sqrt()
    idx = keep.nonzero().squeeze(1)[:rows]
    assert idx.numel() == rows
    return s[idx].contiguous(), None if eps is None else eps[idx].contiguous()


@pytest.mark.parametrize("rows", [17, 256])
@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_fused_actor_loss(kind, rows):
    from gym_uav_collision_avoidance_amd.fused_critic import FusedActorLoss
    pol, crit = actor(kind, 21, device=DEV), critic(kind, 22, device=DEV)
    s, eps = _actor_batch(kind, pol, crit, rows, seed=rows)
    g64, l64, p64 = actor_grads(kind, pol, crit, s, alpha=0.2, noise=eps, dtype=torch.float64)
    g32, _, p32 = actor_grads(kind, pol, crit, s, alpha=0.2, noise=eps, dtype=torch.float32)
    for p in pol.parameters():
        p.grad = torch.ones_like(p)                    # stale: overwritten, not added to
    al = FusedActorLoss(pol, crit)
    assert al.learner == kind
    out = al.backward(s, alpha=0.2, noise=eps)
    torch.cuda.synchronize()
    loss, log_pi = out if kind == "sac" else (out, None)
    assert loss.dim() == 0 and loss.device == DEV and not loss.requires_grad
    for i, (p, r, t) in enumerate(zip(pol.parameters(), g64, g32)):
        _within(p.grad, r, t, f"{kind}/{rows} actor param {i} {tuple(r.shape)}")
    assert abs(float(loss) - float(l64)) <= 1e-6 * abs(float(l64)), (float(loss), float(l64))
    assert all(p.grad is None for p in crit.parameters())
    if kind == "sac":
        assert log_pi.shape == (rows, 1) and not log_pi.requires_grad
        ef, et = float((log_pi.double() - p64).abs().max()), float((p32.double() - p64).abs().max())
        assert ef <= 2 * et, (ef, et)
        # eps drawn from a generator as torch.randn((B, 2)) draws it, alpha as a device tensor
        gen = torch.Generator(device=DEV).manual_seed(77)
        drawn = torch.randn((rows, 2), generator=torch.Generator(device=DEV).manual_seed(77), device=DEV)
        grads = [p.grad.clone() for p in pol.parameters()]
        l1, _ = al.backward(s, alpha=torch.tensor(0.2, device=DEV), generator=gen)
        l2, _ = al.backward(s, alpha=0.2, noise=drawn)
        assert torch.equal(l1, l2)
        al.backward(s, alpha=0.2, noise=eps)
        assert all(torch.equal(p.grad, r) for p, r in zip(pol.parameters(), grads))


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_graph_capture_actor_update_matches_eager(kind):
    from gym_uav_collision_avoidance_amd.fused_critic import FusedActorLoss
    from gym_uav_collision_avoidance_amd.fused_optim import FusedAdam
    g = torch.Generator(device=DEV).manual_seed(41)
    s = torch.randn((256, 10), generator=g, device=DEV)
    eps = torch.randn((256, 2), generator=g, device=DEV) if kind == "sac" else None
    crit = critic(kind, 32, device=DEV)

    def setup():
        pol = actor(kind, 31, device=DEV)
        return pol, FusedActorLoss(pol, crit), FusedAdam(torch.optim.Adam(pol.parameters(), lr=3e-4))

    def step(parts):
        out = parts[1].backward(s, alpha=0.2, noise=eps)
        parts[2].step()
        return out[0] if kind == "sac" else out

    def restart(parts):
        """The weights and optimiser state setup() gives."""
        with torch.no_grad():
            for p, q in zip(parts[0].parameters(), setup()[0].parameters()):
                p.copy_(q)
        for st in parts[2].optimizer.state.values():
            for v in st.values():
                if torch.is_tensor(v):
                    v.zero_()
        parts[2].reload()

    eager = setup()
    el = [step(eager).clone() for _ in range(3)]
    parts = setup()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(parts)                                    # warm-up: creates .grad
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(parts)
    restart(parts)
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, el[i]), i
    for p, q in zip(parts[0].parameters(), eager[0].parameters()):
        assert torch.equal(p, q)


def test_bad_calls_raise():
    from gym_uav_collision_avoidance_amd import policy
    from gym_uav_collision_avoidance_amd.fused_critic import FusedActionGrad, FusedActorLoss, FusedCritic
    m = critic("sac", 30, device=DEV)
    s, a = _batch(m, 64, seed=2)
    with pytest.raises(RuntimeError, match="no kernel compiled"):
        _ag(FusedCritic.from_module(m, precision="bf16")).q_dqda(s, a)
    ag = _ag(m)
    with pytest.raises(ValueError):
        ag.q_dqda(s, a[:63])                                   # rows differ
    with pytest.raises(TypeError):
        ag.q_dqda(s.double(), a)
    with pytest.raises(TypeError):
        ag.q_dqda(s, a.cpu())
    with pytest.raises(ValueError):
        ag.q_dqda(s[:0], a[:0])                                # row count out of range
    with pytest.raises(ValueError):
        ag.q_dqda(s, a, towers=0)
    with pytest.raises(ValueError):
        ag.q_dqda(s, a, towers=4)
    with pytest.raises(ValueError):
        ag.q_dqda(s, a, out=(torch.empty((2, 63), device=DEV), torch.empty((2, 64, 2), device=DEV)))
    with pytest.raises(TypeError):
        FusedActionGrad(policy.TD3Actor().to(DEV))             # not a critic
    d = critic("ddpg", 30, device=DEV)
    dg = _ag(d)
    for mask in (2, 3):
        with pytest.raises(ValueError):
            dg.q_dqda(s, a, towers=mask)                       # a tower DDPG does not have
        with pytest.raises(ValueError):
            dg(s, a, towers=mask)
    # the same from the library itself, on real handles
    lib = _actor_lib.load()
    ptrs = (ctypes.c_void_p * 12)(*[p.data_ptr() for t in towers(d) for p in t])
    out = torch.empty((64, 3), device=DEV)
    for mask in (0, 2, 3):
        rc = lib.uavx_action_grad(dg.critic._h, mask, ptrs, s.data_ptr(), 64, 10, a.data_ptr(), 2, None, out.data_ptr(), None)
        assert rc == _actor_lib.ERR_INVALID_ARG
    rc = lib.uavx_action_grad(dg.critic._h, 1, ptrs, s.data_ptr(), _actor_lib.ACTION_GRAD_MAX_ROWS + 1, 10, a.data_ptr(), 2,
                              None, out.data_ptr(), None)
    assert rc == _actor_lib.ERR_INVALID_ARG
    # q may be NULL: only dqda is written
    j = torch.full((1, 64, 2), NAN, device=DEV)
    rc = lib.uavx_action_grad(dg.critic._h, 1, ptrs, s.data_ptr(), 64, 10, a.data_ptr(), 2, None, j.data_ptr(), None)
    assert rc == _actor_lib.OK and torch.equal(j, dg.q_dqda(s, a)[1])
    # FusedActorLoss: mismatched pair, wrong actor, wrong inputs
    with pytest.raises(TypeError):
        FusedActorLoss(policy.TD3Actor().to(DEV), m)           # a TD3 actor with a SAC critic
    with pytest.raises(TypeError):
        FusedActorLoss(m, m)
    al = FusedActorLoss(policy.GaussianPolicy().to(DEV), ag)
    with pytest.raises(ValueError):
        al.backward(s)                                         # SAC needs alpha
    with pytest.raises(ValueError):
        al.backward(s, alpha=0.2, noise=torch.zeros((63, 2), device=DEV))
    with pytest.raises(TypeError):
        al.backward(s.double(), alpha=0.2)
    with pytest.raises(ValueError):
        al.backward(s[:0], alpha=0.2)

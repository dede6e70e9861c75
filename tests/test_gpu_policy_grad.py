"""FusedPolicyGrad (libuavx_actor.so, include/uavx_policy_grad.h) on the MI355X against float64 and float32 torch autograd
of the trainers' actor losses (tests/action_grad_ref.py) and against the float64 formulas with q and dq/da given
(tests/policy_grad_ref.py): accuracy away from the kinks, every hidden size, the kinks and SAC's clamps themselves, the
backward alone on crafted critic values with ties, the forward alone, ragged rows and strides over NaN memory, determinism,
live weights, graph capture, agreement with FusedActorLoss and argument checks."""
import copy
import ctypes

import pytest
import torch

import policy_grad_ref as ref
from action_grad_ref import actor, actor_grads, sac_sample
from grad_ref import critic, towers
from gym_uav_collision_avoidance_amd import _actor_lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROWS = (1, 15, 16, 17, 255, 256, 257, 4097)
KINDS = ["sac", "td3", "ddpg"]
NAN = float("nan")


def _pg(pol, crit):
    from gym_uav_collision_avoidance_amd.fused_policy_grad import FusedPolicyGrad
    return FusedPolicyGrad(pol, crit)


def _ratio(f, r64, t32, what):
    """(max-abs error of f against float64) / max(2 x torch-f32's own, 2e-6 max|reference|): the project's bound."""
    ef = float((f.double() - r64).abs().max())
    et = float((t32.double() - r64).abs().max())
    top = float(r64.abs().max())
    print(f"{what}: fused {ef:.3e} torch-f32 {et:.3e} max|ref| {top:.3e}")
    bound = max(2 * et, 2e-6 * top)
    return ef / bound if bound > 0 else (0.0 if ef == 0 else float("inf"))


def _within(f, r64, t32, what):
    ratio = _ratio(f, r64, t32, what)
    assert ratio <= 1.0, f"{what}: error / bound {ratio:.3f}"
    return ratio


def _forward(kind, pol, s, eps, dtype):
    """(action, log_pi or None) of torch in `dtype`."""
    p = copy.deepcopy(pol).to(dtype)
    with torch.no_grad():
        if kind == "sac":
            return sac_sample(p, s.to(dtype), eps.to(dtype))
        return p(s.to(dtype)), None


def _check_block(kind, pol, crit, pg, s, eps, what):
    """One backward against float64 autograd of the trainer's loss, under the bound; returns the largest error / bound."""
    g64, l64, p64 = actor_grads(kind, pol, crit, s, alpha=0.2, noise=eps, dtype=torch.float64)
    g32, _, p32 = actor_grads(kind, pol, crit, s, alpha=0.2, noise=eps, dtype=torch.float32)
    rows = s.shape[0]
    a, lp = pg.act(s, noise=eps)
    a64, _ = _forward(kind, pol, s, eps, torch.float64)
    a32, _ = _forward(kind, pol, s, eps, torch.float32)
    assert a.shape == (rows, 2)
    worst = _within(a, a64, a32, f"{what} action")
    for p in pol.parameters():
        p.grad = torch.ones_like(p)                    # stale: overwritten, not added to
    out = pg.backward(s, alpha=0.2, noise=eps)
    torch.cuda.synchronize()
    loss, log_pi = out if kind == "sac" else (out, None)
    assert loss.dim() == 0 and loss.device == DEV and not loss.requires_grad
    for i, (p, r, t) in enumerate(zip(pol.parameters(), g64, g32)):
        worst = max(worst, _within(p.grad, r, t, f"{what} actor param {i} {tuple(r.shape)}"))
    assert abs(float(loss) - float(l64)) <= 1e-6 * abs(float(l64)), (float(loss), float(l64))
    assert all(p.grad is None for p in crit.parameters())
    if kind == "sac":
        assert log_pi.shape == (rows, 1) and lp.shape == (rows, 1) and not log_pi.requires_grad
        worst = max(worst, _within(log_pi, p64, p32, f"{what} log_pi"))
        m64 = float(p64.mean())
        assert abs(float(pg.log_pi_mean) - m64) <= 1e-6 * abs(m64), (float(pg.log_pi_mean), m64)
        assert pg.log_pi_mean.dim() == 0
    else:
        assert lp is None
    return worst


@pytest.mark.parametrize("kind", KINDS)
def test_accuracy_against_float64(kind):
    """Measured on the MI355X, over this test and test_every_hidden_size: the largest error / bound ratio is 0.16 (SAC), 0.14
    (TD3) and 0.31 (DDPG) for the gradients, 0.13 for the action and 0.02 for log_pi; the fused gradients are at most 5.4e-7
    / 2.9e-7 / 3.0e-6 of the tensor maximum from float64, torch-f32's 3.9e-6 / 1.1e-6 / 5.8e-6."""
    pol, crit = actor(kind, 21, device=DEV), critic(kind, 22, device=DEV)
    pg = _pg(pol, crit)
    assert pg.learner == kind
    worst = 0.0
    for rows in ROWS:
        s, eps = ref.batch(kind, pol, crit, rows, seed=rows)
        worst = max(worst, _check_block(kind, pol, crit, pg, s, eps, f"{kind}/{rows}"))
    print(f"{kind}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("kind", KINDS)
def test_every_hidden_size(kind):
    """Partial layer-1 blocks, a single layer-2 unit, fewer unit blocks than waves, and the widest layer 2.

    The critic's output biases are 1: the loss is a mean of float32 q values (the critic launch's output, half an ulp of
    |q| each), so its 1e-6 relative bound can only hold where that mean does not cancel; with the biases' 0.1 N(0, 1) the
    17-row mean of one of these actors came out at 1e-4 of the values it sums."""
    crit = critic(kind, 23, device=DEV)
    with torch.no_grad():
        for t in towers(crit):
            t[5].fill_(1.0)
    worst = 0.0
    for h1 in ((385, 400) if kind == "ddpg" else (241, 256)):
        for h2 in (1, 15, 16, 17, 300, 4096):
            pol = ref.actor_with(kind, h1 + h2, hidden1=h1, hidden2=h2, device=DEV)
            s, eps = ref.batch(kind, pol, crit, 17, seed=h2)
            worst = max(worst, _check_block(kind, pol, crit, _pg(pol, crit), s, eps, f"{kind} {h1}x{h2}"))
    print(f"{kind}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("kind", KINDS)
def test_kinks_follow_torch(kind):
    """s = 0 and every layer-1 bias 0 give z1 = 0 exactly; half the layer-2 biases 0 give z2 = 0 there too.  relu'(0) = 0
    and leaky'(0) = 0.01 as torch: the gradients match torch-f32 autograd."""
    pol, crit = actor(kind, 24, device=DEV), critic(kind, 25, device=DEV)
    l1, l2 = ref.layers(kind, pol)[:2]
    with torch.no_grad():
        l1.bias.zero_()
        l2.bias[::2] = 0.0
    s = torch.zeros((16, 10), device=DEV)
    eps = torch.randn((16, 2), generator=torch.Generator(device=DEV).manual_seed(1), device=DEV) if kind == "sac" else None
    g32, l32, _ = actor_grads(kind, pol, crit, s, alpha=0.2, noise=eps, dtype=torch.float32)
    loss = _pg(pol, crit).backward(s, alpha=0.2, noise=eps)
    loss = loss[0] if kind == "sac" else loss
    torch.cuda.synchronize()
    for i, (p, t) in enumerate(zip(pol.parameters(), g32)):
        err, top = float((p.grad - t).abs().max()), float(t.abs().max())
        assert err <= 1e-5 * top, (i, err, top)
    assert abs(float(loss) - float(l32)) <= 1e-5 * abs(float(l32))


def test_log_std_clamp_edges_follow_torch():
    """log_std_linear.weight = 0 makes the raw log-std its bias on every row.  torch.clamp passes its gradient at equality
    (2.0 and -20.0) and blocks it outside (the next float above 2, and 2.5)."""
    crit = critic("sac", 27, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    s = torch.randn((17, 10), generator=g, device=DEV)
    eps = torch.randn((17, 2), generator=g, device=DEV)
    above = float(torch.nextafter(torch.tensor(2.0), torch.tensor(3.0)))
    for bias, passes in ((2.0, True), (-20.0, True), (above, False), (2.5, False)):
        pol = actor("sac", 26, device=DEV)
        with torch.no_grad():
            pol.log_std_linear.weight.zero_()
            pol.log_std_linear.bias.fill_(bias)
        assert float(pol.log_std_linear.bias.detach()[0]) == bias
        g64, _, _ = actor_grads("sac", pol, crit, s, alpha=0.2, noise=eps, dtype=torch.float64)
        g32, _, _ = actor_grads("sac", pol, crit, s, alpha=0.2, noise=eps, dtype=torch.float32)
        _pg(pol, crit).backward(s, alpha=0.2, noise=eps)
        torch.cuda.synchronize()
        gw, gb = pol.log_std_linear.weight.grad, pol.log_std_linear.bias.grad
        if passes:
            assert bool((gb != 0).all()) and bool((g64[7] != 0).all()) and float(gw.abs().max()) > 0
            _within(gb, g64[7], g32[7], f"log_std bias {bias} db")
            _within(gw, g64[6], g32[6], f"log_std bias {bias} dW")
        else:
            assert bool((g64[7] == 0).all()) and bool((g64[6] == 0).all())
            assert bool((gb == 0).all()) and bool((gw == 0).all())


@pytest.mark.parametrize("kind", KINDS)
def test_backward_from_crafted_q_and_jacobian(kind):
    """q and dq/da random, not a critic's.  SAC: a quarter of the rows have q1 == q2 bitwise, the others are split between
    < and >, and J1 != J2 everywhere, so the tie rows tell 1/2 : 1/2 from either one-sided choice."""
    rows, T = 64, 1 if kind == "ddpg" else 2
    pol, crit = actor(kind, 28, device=DEV), critic(kind, 29, device=DEV)
    s, eps = ref.batch(kind, pol, crit, rows, seed=6)
    g = torch.Generator(device=DEV).manual_seed(7)
    q = torch.randn((T, rows), generator=g, device=DEV)
    J = torch.randn((T, rows, 2), generator=g, device=DEV)
    if T == 2:
        q[1, 0::4] = q[0, 0::4]
        q[1, 1::4] = q[0, 1::4] + 0.5
        q[1, 2::4] = q[0, 2::4] - 0.5
        assert int((q[0] == q[1]).sum()) == 16 and int((q[0] < q[1]).sum()) >= 16 and int((q[0] > q[1]).sum()) >= 16
        assert bool((J[0] != J[1]).all())
    pg = _pg(pol, crit)
    a, _ = pg.act(s, noise=eps)
    out = pg.backward_from(s, q, J, alpha=0.2)
    torch.cuda.synchronize()
    loss = out[0] if kind == "sac" else out
    r64 = ref.analytic(kind, pol, s, q, J, alpha=0.2, noise=eps, dtype=torch.float64)
    r32 = ref.analytic(kind, pol, s, q, J, alpha=0.2, noise=eps, dtype=torch.float32)
    for i, (p, r, t) in enumerate(zip(pol.parameters(), r64["grads"], r32["grads"])):
        _within(p.grad, r, t, f"{kind} crafted param {i}")
    assert abs(float(loss) - float(r64["loss"])) <= 1e-6 * abs(float(r64["loss"]))
    _within(a, r64["action"], r32["action"], f"{kind} crafted action")
    if kind == "sac":
        for tie in (0.0, 1.0):
            one = ref.analytic(kind, pol, s, q, J, alpha=0.2, noise=eps, tie=tie)["grads"]
            ratios = [_ratio(o, r, t, f"tie weight {tie} param {i}")
                      for i, (o, r, t) in enumerate(zip(one, r64["grads"], r32["grads"]))]
            assert max(ratios) > 1.0, ratios
    with pytest.raises(RuntimeError):
        pg.backward_from(s[:32], q[:, :32].contiguous(), J[:, :32].contiguous(), alpha=0.2)   # no act() on these rows


@pytest.mark.parametrize("kind", KINDS)
def test_act_alone(kind):
    pol, crit = actor(kind, 30, device=DEV), critic(kind, 31, device=DEV)
    s, eps = ref.batch(kind, pol, crit, 257, seed=8)
    pg = _pg(pol, crit)
    a, lp = pg.act(s, noise=eps)
    a64, p64 = _forward(kind, pol, s, eps, torch.float64)
    a32, p32 = _forward(kind, pol, s, eps, torch.float32)      # FusedActorLoss's torch forward
    _within(a, a64, a32, f"{kind} act")
    assert all(p.grad is None for p in pol.parameters())
    if kind != "sac":
        assert lp is None
        return
    _within(lp, p64, p32, "sac act log_pi")
    a, lp = a.clone(), lp.clone()
    # eps drawn from a generator as torch.randn((B, 2)) draws it
    drawn = torch.randn((257, 2), generator=torch.Generator(device=DEV).manual_seed(77), device=DEV)
    a1, l1 = (x.clone() for x in pg.act(s, generator=torch.Generator(device=DEV).manual_seed(77)))
    a2, l2 = pg.act(s, noise=drawn)
    assert torch.equal(a1, a2) and torch.equal(l1, l2) and not torch.equal(a1, a)
    # alpha as a device tensor and as a float
    la, _ = pg.backward(s, alpha=0.2, noise=eps)
    ga = [la.clone()] + [p.grad.clone() for p in pol.parameters()]
    lb, _ = pg.backward(s, alpha=torch.tensor(0.2, device=DEV), noise=eps)
    assert all(torch.equal(x, y) for x, y in zip(ga, [lb] + [p.grad for p in pol.parameters()]))
    lc, _ = pg.backward(s, alpha=torch.tensor([0.3], device=DEV), noise=eps)
    assert not torch.equal(lc, ga[0])


@pytest.mark.parametrize("kind", ["sac", "ddpg"])
def test_ragged_rows_and_strides_over_nan_memory(kind):
    """The ABI itself on guarded buffers: state rows of stride 16 whose six unused columns hold NaN, the rows after the last
    one NaN too, and every output and the workspace between NaN guards."""
    lib = _actor_lib.load()
    K = {"sac": _actor_lib.SAC, "ddpg": _actor_lib.DDPG}[kind]
    pol, crit = actor(kind, 32, device=DEV), critic(kind, 33, device=DEV)
    pg = _pg(pol, crit)
    ps = ref.params(kind, pol)
    h1, h2, T, G = ps[0].shape[0], ps[2].shape[0], 1 if kind == "ddpg" else 2, 64
    pp = (ctypes.c_void_p * 8)(*([p.data_ptr() for p in ps] + [None] * (8 - len(ps))))
    for rows in (1, 17):
        s, eps = ref.batch(kind, pol, crit, rows, seed=9)
        out = pg.backward(s, alpha=0.2, noise=eps)
        torch.cuda.synchronize()
        want = [x.clone() for x in (out if kind == "sac" else (out,))] + [p.grad.clone() for p in ps]
        want_a = pg._action[:rows * 2].clone()
        assert all(bool(torch.isfinite(x).all()) for x in want)
        wide = torch.full((rows + 8, 16), NAN, device=DEV)
        wide[:rows, :10] = s
        sv = wide[:rows, :10]
        eb = torch.full((rows + 8, 2), NAN, device=DEV)
        if kind == "sac":
            eb[:rows] = eps
        need = pg.workspace_bytes(rows)
        assert need % 256 == 0

        def guarded(n):
            t = torch.full((2 * G + n,), NAN, device=DEV)
            return t, t[G:G + n]

        bufs = {k: guarded(n) for k, n in (("a", rows * 2), ("lp", rows), ("q", T * rows), ("j", T * rows * 2),
                                           ("loss", 1), ("lpm", 1), ("ws", need // 4))}
        gs = [guarded(p.numel()) for p in ps]
        gp = (ctypes.c_void_p * 8)(*([g[1].data_ptr() for g in gs] + [None] * (8 - len(ps))))
        ws = bufs["ws"][1]
        sac = kind == "sac"
        rc = lib.uavx_policy_grad_forward(K, h1, h2, pp, sv.data_ptr(), rows, 16, eb.data_ptr() if sac else None,
                                          bufs["a"][1].data_ptr(), bufs["lp"][1].data_ptr() if sac else None, ws.data_ptr(),
                                          need, None)
        assert rc == _actor_lib.OK
        pg.critic.q_dqda(sv, bufs["a"][1].view(rows, 2), towers=3 if sac else 1,
                         out=(bufs["q"][1].view(T, rows), bufs["j"][1].view(T, rows, 2)))
        rc = lib.uavx_policy_grad_backward(K, h1, h2, pp, sv.data_ptr(), rows, 16, bufs["q"][1].data_ptr(),
                                           bufs["j"][1].data_ptr(), rows, 0.2, None, gp, bufs["loss"][1].data_ptr(),
                                           bufs["lpm"][1].data_ptr() if sac else None, ws.data_ptr(), need, None)
        assert rc == _actor_lib.OK
        torch.cuda.synchronize()
        for name, (full, _) in list(bufs.items()) + [(f"grad{i}", g) for i, g in enumerate(gs)]:
            assert bool(torch.isnan(full[:G]).all()) and bool(torch.isnan(full[-G:]).all()), name
        got = [bufs["loss"][1][0]] + ([bufs["lp"][1].view(rows, 1)] if sac else []) + [g[1].view(p.shape) for g, p in zip(gs, ps)]
        assert len(got) == len(want)
        for x, r in zip(got, want):
            assert torch.equal(x, r)
        assert torch.equal(bufs["a"][1], want_a)
        if sac:
            assert float(bufs["lpm"][1][0]) == float(pg.log_pi_mean)
        else:                                          # TD3 / DDPG: log_pi and its mean are not written
            assert bool(torch.isnan(bufs["lp"][1]).all()) and bool(torch.isnan(bufs["lpm"][1]).all())


@pytest.mark.parametrize("kind", KINDS)
def test_determinism_and_live_weights(kind):
    pol, crit = actor(kind, 34, device=DEV), critic(kind, 35, device=DEV)
    s, eps = ref.batch(kind, pol, crit, 257, seed=10)
    pg = _pg(pol, crit)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-2)
    l1 = pg.backward(s, alpha=0.2, noise=eps)
    first = [(l1[0] if kind == "sac" else l1).clone()] + [p.grad.clone() for p in pol.parameters()]
    l2 = pg.backward(s, alpha=0.2, noise=eps)
    again = [l2[0] if kind == "sac" else l2] + [p.grad for p in pol.parameters()]
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    # what the trainers do between two actor updates: in place, and nothing is refreshed
    opt.step()
    g = torch.Generator(device=DEV).manual_seed(2)
    with torch.no_grad():
        for p in crit.parameters():
            p.add_(torch.randn(p.shape, generator=g, device=DEV) * 0.01)
    s, eps = ref.batch(kind, pol, crit, 257, seed=10)          # the new weights move the kinks
    _check_block(kind, pol, crit, pg, s, eps, f"{kind} live")
    assert not torch.equal(first[1], next(pol.parameters()).grad)


@pytest.mark.parametrize("kind", KINDS)
def test_graph_capture_actor_update_matches_eager(kind):
    from gym_uav_collision_avoidance_amd.fused_optim import FusedAdam
    g = torch.Generator(device=DEV).manual_seed(41)
    s = torch.randn((256, 10), generator=g, device=DEV)
    eps = torch.randn((256, 2), generator=g, device=DEV) if kind == "sac" else None
    crit = critic(kind, 32, device=DEV)

    def setup(reserve=True):
        pol = actor(kind, 31, device=DEV)
        pg = _pg(pol, crit)
        if reserve:
            pg.reserve(256)
        return pol, pg, FusedAdam(torch.optim.Adam(pol.parameters(), lr=3e-4))

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
    bare = setup(reserve=False)[1]                     # no workspace yet: a capture cannot allocate one
    marker = torch.zeros(1, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="reserve"):
            bare.backward(s, alpha=0.2, noise=eps)
        out = step(parts)
        marker.add_(1.0)
    restart(parts)
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, el[i]), i
    assert float(marker) == 3.0
    for p, q in zip(parts[0].parameters(), eager[0].parameters()):
        assert torch.equal(p, q)


@pytest.mark.parametrize("kind", KINDS)
def test_agrees_with_fused_actor_loss(kind):
    from gym_uav_collision_avoidance_amd.fused_critic import FusedActionGrad, FusedActorLoss
    pol, crit = actor(kind, 36, device=DEV), critic(kind, 37, device=DEV)
    s, eps = ref.batch(kind, pol, crit, 256, seed=11)
    g64, l64, _ = actor_grads(kind, pol, crit, s, alpha=0.2, noise=eps, dtype=torch.float64)
    g32, _, _ = actor_grads(kind, pol, crit, s, alpha=0.2, noise=eps, dtype=torch.float32)
    ag = FusedActionGrad(crit)                         # one critic launch object serves both blocks
    for name, block in (("FusedActorLoss", FusedActorLoss(pol, ag)), ("FusedPolicyGrad", _pg(pol, ag))):
        for p in pol.parameters():
            p.grad = None
        out = block.backward(s, alpha=0.2, noise=eps)
        torch.cuda.synchronize()
        loss = out[0] if kind == "sac" else out
        for i, (p, r, t) in enumerate(zip(pol.parameters(), g64, g32)):
            _within(p.grad, r, t, f"{kind} {name} param {i}")
        assert abs(float(loss) - float(l64)) <= 1e-6 * abs(float(l64))


def test_bad_calls_raise():
    from gym_uav_collision_avoidance_amd import policy
    from gym_uav_collision_avoidance_amd.fused_critic import FusedCritic
    pol, crit = actor("sac", 38, device=DEV), critic("sac", 39, device=DEV)
    pg = _pg(pol, crit)
    s = torch.randn((64, 10), device=DEV)
    eps = torch.randn((64, 2), device=DEV)
    with pytest.raises(ValueError):
        pg.backward(s)                                         # SAC needs alpha
    with pytest.raises(TypeError):
        pg.backward(s.double(), alpha=0.2)
    with pytest.raises(TypeError):
        pg.backward(s.cpu(), alpha=0.2)
    with pytest.raises(ValueError):
        pg.backward(s[:, :9], alpha=0.2)
    with pytest.raises(ValueError):
        pg.backward(s[:0], alpha=0.2)                          # rows 0
    with pytest.raises(ValueError):
        pg.backward(s, alpha=0.2, noise=eps[:63])
    with pytest.raises(TypeError):
        pg.backward(s, alpha=0.2, noise=eps.double())
    with pytest.raises(TypeError):
        pg.backward(s, alpha=torch.tensor(0.2))                # alpha on the host
    with pytest.raises(ValueError):
        pg.backward(s, alpha=torch.tensor([0.2, 0.3], device=DEV))
    pg.act(s, noise=eps)
    q, j = torch.zeros((2, 64), device=DEV), torch.zeros((2, 64, 2), device=DEV)
    with pytest.raises(ValueError):
        pg.backward_from(s, q[:1], j, alpha=0.2)               # one tower of two
    with pytest.raises(TypeError):
        pg.backward_from(s, q.double(), j, alpha=0.2)
    with pytest.raises(ValueError):
        pg.backward_from(s, q, j)
    assert all(p.grad is None for p in pol.parameters())       # nothing ran
    with pytest.raises(TypeError):
        _pg(policy.TD3Actor().to(DEV), crit)                   # a TD3 actor with a SAC critic
    with pytest.raises(TypeError):
        _pg(crit, crit)
    with pytest.raises(ValueError):
        _pg(policy.GaussianPolicy(), crit)                     # a CPU actor
    with pytest.raises(RuntimeError, match="no kernel compiled"):
        _pg(pol, FusedCritic.from_module(crit, precision="bf16")).backward(s, alpha=0.2)
    with pytest.raises(RuntimeError):
        _pg(policy.GaussianPolicy(hidden=128).to(DEV), crit)   # no register tile of that width
    with pytest.raises(AttributeError):
        _pg(actor("td3", 1, device=DEV), critic("td3", 2, device=DEV)).log_pi_mean

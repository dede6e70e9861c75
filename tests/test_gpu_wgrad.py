"""FusedCriticLoss.backward(weight=, q_out=) (libuavx_actor.so, include/uavx_wcritic_grad.h) on the MI355X: a
weight of 1 is the unweighted call bit for bit, the weight enters once and linearly, a zero-weight row is a padded row,
random weights against float64 autograd of the weighted loss (tests/wgrad_ref.py) within §14's bounds, graph capture, and
the learners' `per_beta` keyword: the sampler's weights reach the critic loss, the gradient's q reaches the priorities,
eager equals captured, and per_beta = 0 changes nothing."""
import functools

import numpy as np
import pytest
import torch

import wgrad_ref
from grad_ref import autograd as unweighted_autograd
from test_gpu_critic_grad import _batch
from wgrad_ref import critic, params

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROWS = (1, 15, 16, 17, 64, 65, 257, 1040)          # block edges at 16; the split-K slice count changes above 64
SHAPES = {"sac": [(h1, h2) for h1 in (241, 256) for h2 in (1, 17, 256)],
          "td3": [(h1, h2) for h1 in (241, 256) for h2 in (1, 17, 256)],
          "ddpg": [(h1, h2) for h1 in (385, 400) for h2 in (1, 300)]}


def _closs(m, loss=None):
    from gym_uav_collision_avoidance_amd.fused_critic import FusedCriticLoss
    return FusedCriticLoss(m, loss=loss)


@functools.lru_cache(maxsize=None)
def _case(kind, h1=None, h2=None, rows=max(ROWS)):
    """(critic, s, a, y) kept away from the activation and L1 kinks (test_gpu_critic_grad._batch); a prefix of the rows is
    as far from them.  Made once and never written to."""
    m = critic(kind, 40 + (h1 or 0) + (h2 or 0), hidden1=h1, hidden2=h2, device=DEV)
    return (m,) + _batch(m, rows, seed=5 + (h2 or 0))


def _run(cl, m, s, a, y, **kw):
    """One backward -> (bits of every .grad and of the losses, as int32 tensors)."""
    ls = cl.backward(s, a, y, **kw)
    ls = list(ls) if isinstance(ls, tuple) else [ls]
    return [p.grad.clone().view(torch.int32) for p in params(m)] + [l.clone().view(torch.int32) for l in ls]


def _same(got, want):
    return len(got) == len(want) and all(torch.equal(x, w) for x, w in zip(got, want))


def _floats(bits):
    return [b.view(torch.float32) for b in bits]


# ---- 1. weight 1 is the unweighted call ----------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["mse", "l1"])
@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_weight_one_is_the_unweighted_call(kind, loss):
    for h1, h2 in SHAPES[kind]:
        m, S, A, Y = _case(kind, h1, h2)
        cl = _closs(m, loss)
        T = cl.critic.towers
        ones = torch.ones(max(ROWS), device=DEV)
        for rows in ROWS:
            s, a, y = S[:rows], A[:rows], Y[:rows]
            want = _run(cl, m, s, a, y)
            q0 = torch.full((T, rows), float("nan"), device=DEV)
            q1 = torch.full((T, rows), float("nan"), device=DEV)
            assert _same(_run(cl, m, s, a, y, q_out=q0), want), (h1, h2, rows, "weight=None")
            assert _same(_run(cl, m, s, a, y, weight=ones[:rows]), want), (h1, h2, rows, "ones")
            assert _same(_run(cl, m, s, a, y, weight=ones[:rows].unsqueeze(1), q_out=q1), want), (h1, h2, rows, "ones, q")
            assert torch.equal(q0, q1) and bool(torch.isfinite(q0).all())
        cl.close()


def test_weight_one_on_strided_inputs():
    for kind in ("sac", "ddpg"):
        m, S, A, Y = _case(kind)
        rows = 257
        cl = _closs(m)
        want = _run(cl, m, S[:rows], A[:rows], Y[:rows])
        s = torch.full((rows, 40), float("nan"), device=DEV)[:, :10]
        a = torch.full((rows, 8), float("nan"), device=DEV)[:, :2]
        y = torch.full((rows, 3), float("nan"), device=DEV)[:, 1]
        w = torch.full((rows, 2), float("nan"), device=DEV)[:, 1]
        s.copy_(S[:rows]); a.copy_(A[:rows]); y.copy_(Y[:rows]); w.fill_(1.0)
        assert s.stride(0) == 40 and a.stride(0) == 8 and y.stride(0) == 3 and w.stride(0) == 2
        q = torch.empty((cl.critic.towers, rows), device=DEV)
        assert _same(_run(cl, m, s, a, y, weight=w, q_out=q), want)
        assert _same(_run(cl, m, s, a, y.unsqueeze(1), weight=w.unsqueeze(1)), want)
        cl.close()


# ---- 2. the weight enters once, linearly ---------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["mse", "l1"])
@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_weight_scales_everything_exactly(kind, loss):
    """Scaling by a power of two is exact through every f32 and f64 step (inputs of ordinary magnitude, nothing near
    denormal): w = 0.5 halves and w = 2 doubles every gradient and loss bit for bit.  A squared or forgotten weight fails."""
    m, S, A, Y = _case(kind)
    cl = _closs(m, loss)
    for rows in (65, 257):
        s, a, y = S[:rows], A[:rows], Y[:rows]
        one = _floats(_run(cl, m, s, a, y, weight=torch.ones(rows, device=DEV)))
        assert all(float(x.abs().max()) > 1e-12 for x in one)
        for scale in (0.5, 2.0):
            got = _run(cl, m, s, a, y, weight=torch.full((rows,), scale, device=DEV))
            assert _same(got, [(x * scale).view(torch.int32) for x in one]), (rows, scale)
    cl.close()


# ---- 3. a zero-weight row is a padded row --------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["mse", "l1"])
@pytest.mark.parametrize("kind", ["sac", "ddpg"])
def test_zero_weight_rows_are_padded_rows(kind, loss):
    """B = 32 with w = [1]·16 + [0]·16 against the unweighted batch of the first 16 rows: 2/32 (1/32) is half of 2/16
    (1/16), both have one split-K slice, and the second block sums exact zeros: every gradient and loss is exactly half."""
    m, S, A, Y = _case(kind)
    cl = _closs(m, loss)
    half = _floats(_run(cl, m, S[:16], A[:16], Y[:16]))
    w = torch.cat([torch.ones(16, device=DEV), torch.zeros(16, device=DEV)])
    q = torch.empty((cl.critic.towers, 32), device=DEV)
    got = _floats(_run(cl, m, S[:32], A[:32], Y[:32], weight=w, q_out=q))
    for x, h in zip(got, half):
        assert float(h.abs().max()) > 0 and torch.equal(x, 0.5 * h)
    # q is written for the zero-weight rows too
    q16 = torch.empty((cl.critic.towers, 16), device=DEV)
    cl.backward(S[:16], A[:16], Y[:16], q_out=q16)
    assert torch.equal(q[:, :16], q16) and bool(torch.isfinite(q).all())
    cl.close()


# ---- 4. random weights against float64 ------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["mse", "l1"])
@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_random_weights_against_float64(kind, loss):
    """§14's bounds on the weighted loss: each parameter's max-abs error <= max(2 x torch-f32 autograd's own, 2e-6 max|g64|),
    losses to 1e-6 relative, q_out within max(2 x torch-f32's forward error, 2e-6 max|q64|).  Weights in [0.05, 1]."""
    m, S, A, Y = _case(kind, rows=4096)
    cl = _closs(m, loss)
    T = cl.critic.towers
    for rows in (1, 17, 257, 4096):
        s, a, y = S[:rows], A[:rows], Y[:rows]
        w = torch.rand(rows, generator=torch.Generator(device=DEV).manual_seed(rows), device=DEV) * 0.95 + 0.05
        q = torch.empty((T, rows), device=DEV)
        got = _floats(_run(cl, m, s, a, y, weight=w, q_out=q))
        gf, lf = got[:6 * T], got[6 * T:]
        g64, l64, q64 = wgrad_ref.autograd(m, s, a, y, w, loss, torch.float64)
        g32, _, q32 = wgrad_ref.autograd(m, s, a, y, w, loss, torch.float32)
        for i, (f, r, t) in enumerate(zip(gf, g64, g32)):
            ef, et = float((f.double() - r).abs().max()), float((t.double() - r).abs().max())
            print(f"{kind}/{loss}/{rows} param {i}: fused {ef:.3e} torch-f32 {et:.3e} max|g| {float(r.abs().max()):.3e}")
            assert ef <= max(2 * et, 2e-6 * float(r.abs().max())), (rows, i, ef, et)
        for f, r in zip(lf, l64):
            assert abs(float(f) - float(r)) <= 1e-6 * abs(float(r)), (rows, float(f), float(r))
        for t in range(T):
            ef, et = float((q[t].double() - q64[t]).abs().max()), float((q32[t].double() - q64[t]).abs().max())
            print(f"{kind}/{loss}/{rows} q{t}: fused {ef:.3e} torch-f32 {et:.3e} max|q| {float(q64[t].abs().max()):.3e}")
            assert ef <= max(2 * et, 2e-6 * float(q64[t].abs().max())), (rows, t, ef, et)
        # the weights matter here: the unweighted gradients are far outside that bound
        if rows >= 17:
            u64, _ = unweighted_autograd(m, s, a, y, loss, torch.float64)
            assert float((u64[2] - g64[2]).abs().max()) > 1e-3 * float(g64[2].abs().max())
    cl.close()


# ---- 5. graph capture -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["sac", "ddpg"])
def test_captured_weighted_call_equals_eager(kind):
    m, S, A, Y = _case(kind)
    rows = 257
    s, a, y = S[:rows], A[:rows], Y[:rows]
    w = torch.rand(rows, generator=torch.Generator(device=DEV).manual_seed(3), device=DEV) * 0.95 + 0.05
    eager = _closs(m)
    T = eager.critic.towers
    qe = torch.empty((T, rows), device=DEV)
    want = _run(eager, m, s, a, y, weight=w, q_out=qe)         # also loads every kernel before the capture
    torch.cuda.synchronize()
    cl = _closs(m).reserve(rows)
    for p in m.parameters():
        p.grad.zero_()
    qg = torch.zeros((T, rows), device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ls = cl.backward(s, a, y, weight=w, q_out=qg)
    assert not bool(qg.any())                                  # the capture itself ran nothing
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        ls_ = list(ls) if isinstance(ls, tuple) else [ls]
        got = [p.grad.view(torch.int32) for p in params(m)] + [l.view(torch.int32) for l in ls_]
        assert _same(got, want) and torch.equal(qg, qe)
    other = _closs(m)                                          # no reserve(): the workspace cannot appear during a capture
    with pytest.raises(RuntimeError, match="before a graph capture"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            other.backward(s, a, y, weight=w, q_out=qg)
    for c in (eager, cl, other):
        c.close()


def test_bad_weighted_calls_are_refused_on_the_host():
    from gym_uav_collision_avoidance_amd.fused_critic import FusedCritic
    m, S, A, Y = _case("sac")
    s, a, y = S[:64], A[:64], Y[:64]
    cl = _closs(m)
    w, q = torch.ones(64, device=DEV), torch.empty((2, 64), device=DEV)
    before = _run(cl, m, s, a, y)
    for kw, exc in ((dict(weight=w[:63]), ValueError), (dict(weight=w.double()), TypeError), (dict(weight=w.cpu()), TypeError),
                    (dict(weight=torch.ones((64, 2), device=DEV)), ValueError), (dict(weight=[1.0] * 64), TypeError),
                    (dict(weight=w[:1].expand(64)), ValueError),            # a stride of 0
                    (dict(q_out=q[:1]), ValueError), (dict(q_out=torch.empty((64, 2), device=DEV).T), ValueError),
                    (dict(q_out=q.double()), TypeError), (dict(q_out=torch.empty((2, 63), device=DEV)), ValueError)):
        with pytest.raises(exc, match="uavx:"):
            cl.backward(s, a, y, **kw)
    with pytest.raises(RuntimeError, match="uavx: .*f32 only"):
        _closs(FusedCritic.from_module(m, precision="bf16")).backward(s, a, y, weight=w)
    assert _same(_run(cl, m, s, a, y), before)
    cl.close()


# ---- 6. learners ----------------------------------------------------------------------------------------------------------
LE, LN, LT = 16, 4, 32


@pytest.fixture(scope="module")
def memory():
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    env = BatchedMultiUAVWorld2D(LE, num_agents=LN, device=DEV, seed=3)
    mem = DeviceReplay(env, horizon=LT)
    mem.begin(env.reset())
    g = torch.Generator(device=DEV).manual_seed(103)
    for _ in range(LT + 3):
        mem.action_slot().copy_(torch.rand((LE, LN, 2), generator=g, device=DEV) * 2 - 1)
        mem.step(polar=True, auto_reset="agent0_done", step_cap=12)
    yield mem
    env.close()


def _learner(kind, **kw):
    from gym_uav_collision_avoidance_amd import learners
    cls = {"sac": learners.FusedSAC, "td3": learners.FusedTD3, "ddpg": learners.FusedDDPG}[kind]
    torch.manual_seed(11)                                             # the same initial weights every time
    return cls(device=DEV, generator=torch.Generator(device=DEV).manual_seed(77), **kw)


def _table(agent):
    torch.cuda.synchronize()
    return agent._sampler.priorities.cpu().numpy().copy(), agent._sampler.record()


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_weighted_learner_eager_equals_captured(kind, memory):
    from gym_uav_collision_avoidance_amd.prioritized_replay import PrioritizedReplaySampler
    eager = _learner(kind, prioritized=0.6, per_beta=0.4, memory=memory)
    sampler = eager._sampler
    assert isinstance(sampler, PrioritizedReplaySampler) and sampler.alpha == 0.6 and sampler.beta == 0.4 == eager.per_beta
    batches, calls, fed = [], [], []
    sample, backward, update = sampler.sample, eager._closs.backward, sampler.update_priorities

    def spy_sample(*a, **kw):
        batches.append(sample(*a, **kw))
        return batches[-1]

    def spy_backward(s, a, y, weight=None, q_out=None):
        out = backward(s, a, y, weight=weight, q_out=q_out)
        calls.append((weight, q_out, None if weight is None else weight.clone(), None if q_out is None else q_out.clone()))
        return out

    def spy_update(key, q, y=None, **kw):
        fed.append((key, q, q.clone()))
        return update(key, q, y, **kw)

    launches, q_dqda = [], eager._pgrad.critic.q_dqda

    def spy_q_dqda(*a, **kw):
        launches.append(kw.get("out"))
        return q_dqda(*a, **kw)

    sampler.sample, eager._closs.backward, sampler.update_priorities = spy_sample, spy_backward, spy_update
    eager._pgrad.critic.q_dqda = spy_q_dqda
    first = _table(eager.attach(memory))[0]
    for _ in range(6):
        eager.update_parameters(None, 64)
    want_table, want_rec = _table(eager)
    want_log = eager.losses()
    assert len(batches) == len(calls) == len(fed) == 6
    # q_dqda runs in the actor update alone (TD3: every second update): no feedback launch, nothing writes the feedback's q
    assert len(launches) == (3 if kind == "td3" else 6) and not any(o is not None and o[0] is calls[0][1] for o in launches)
    T = eager._closs.critic.towers
    for batch, (w, q, w_then, q_then), (key, q_fed, q_fed_then) in zip(batches, calls, fed):
        assert w is batch[5] and key is batch[6]                  # the sampler's weight tensor, the sampler's keys
        assert tuple(q.shape) == (T, 64) and q_fed is q           # the q the gradient wrote is the q the priorities get
        assert torch.equal(q_then, q_fed_then) and bool(torch.isfinite(q_then).all())
        assert 0.0 < float(w_then.min()) <= float(w_then.max()) <= 1.0
    assert any(float(c[2].min()) < 1.0 for c in calls)            # beta = 0.4 on moved priorities: real weights
    assert (want_table != first).any() and want_log.shape == (6, 8) and np.isfinite(want_log).all()
    # captured: the same six updates, bit for bit (TD3: two graphs)
    graphed = _learner(kind, prioritized=0.6, per_beta=0.4, memory=memory)
    graphed.capture(64)
    assert len(graphed._graphs) == (2 if kind == "td3" else 1)
    graphed.run(6)
    got_table, got_rec = _table(graphed)
    got_log = graphed.losses()
    assert got_log.shape == (6, 8) and np.array_equal(got_log.view(np.int32), want_log.view(np.int32))
    assert np.array_equal(got_table, want_table) and got_rec == want_rec
    # the captured update follows set_per_beta: beta lives in a device slot
    for agent in (eager, graphed):
        assert agent.set_per_beta(1.0) is agent and agent.per_beta == 1.0 == agent._sampler.beta
    for _ in range(3):
        eager.update_parameters(None, 64)
    graphed.run(3)
    assert np.array_equal(graphed.losses().view(np.int32), eager.losses().view(np.int32))
    a, b = _table(graphed), _table(eager)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert float(graphed._sampler._beta) == 1.0 and float(calls[-1][2].min()) < 1.0
    # an explicit weight without a key weights the loss and leaves the table alone
    batch = memory.sample(64, generator=torch.Generator(device=DEV).manual_seed(1))
    n = len(calls)
    w = torch.rand(64, device=DEV) * 0.5 + 0.5
    eager.update_batch(*batch, weight=w)
    assert np.array_equal(_table(eager)[0], b[0]) and len(calls) == n + 1 and calls[-1][0] is w and calls[-1][1] is None
    assert len(fed) == 9
    with pytest.raises(ValueError, match="uavx: weight must be"):
        eager.update_batch(*batch, weight=w[:7])
    with pytest.raises(ValueError, match=r"per_beta in \[0, 1\]"):
        eager.set_per_beta(1.5)
    for agent in (eager, graphed):
        agent.close()


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_per_beta_zero_changes_nothing(kind, memory):
    plain, keyword = _learner(kind, memory=memory, prioritized=0.6), _learner(kind, memory=memory, prioritized=0.6, per_beta=0.0)
    assert keyword._sampler.beta == 0.0 == plain._sampler.beta and keyword.per_beta == 0.0
    seen = []
    inner = keyword._closs.backward
    keyword._closs.backward = lambda *a, **kw: (seen.append((len(a), kw)), inner(*a, **kw))[1]
    for agent in (plain, keyword):
        for _ in range(6):
            agent.update_parameters(None, 64)
    a, b = plain.losses(), keyword.losses()
    assert a.shape == (6, 8) and np.array_equal(a.view(np.int32), b.view(np.int32))
    assert np.array_equal(_table(plain)[0], _table(keyword)[0])
    assert seen == [(3, {})] * 6                                      # the unweighted call, as before
    with pytest.raises(ValueError, match="set_per_beta needs"):
        keyword.set_per_beta(0.5)
    for agent in (plain, keyword):
        agent.close()

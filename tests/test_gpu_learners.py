"""FusedSAC / FusedTD3 / FusedDDPG (gym_uav_collision_avoidance_amd/learners.py) and uavx_learner_tail
(include/uavx_learner.h) on the MI355X: the whole fused update against the reference's own update_parameters (the fixtures
of tests/golden/make_learner_updates.py) under the project's distance rule, the tail launch alone against its float64
statement, the update against the same launches composed by hand, graph replay against eager updates, checkpoints, and
SAC's delayed target update."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import learner_ref as lr
from gym_uav_collision_avoidance_amd import _actor_lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAN = float("nan")
NETS = {"sac": ("policy", "critic", "critic_target"), "td3": ("actor", "actor_target", "critic", "critic_target"),
        "ddpg": ("actor", "actor_target", "critic", "critic_target")}


def _cls(kind):
    from gym_uav_collision_avoidance_amd import learners
    return {"sac": learners.FusedSAC, "td3": learners.FusedTD3, "ddpg": learners.FusedDDPG}[kind]


def _learner(kind, **kw):
    """A learner at the recipe weights of tests/learner_ref.py."""
    return lr.load_recipe(_cls(kind)(device=DEV, **kw), kind).refresh()


def _tensors(agent, kind):
    out = {f"{k}.{n}": p.detach() for k in NETS[kind] for n, p in getattr(agent, k).named_parameters()}
    if kind == "sac" and agent.automatic_entropy_tuning:
        out["log_alpha"] = agent.log_alpha.detach()
    return out


def _state(agent, kind):
    """Every tensor an update moves, cloned: parameters, targets, optimiser moments, SAC's alpha."""
    out = [p.detach().clone() for p in _tensors(agent, kind).values()]
    opts = [getattr(agent, n) for n in ("critic_optim", "policy_optim", "alpha_optim", "actor_optimizer", "critic_optimizer")
            if hasattr(agent, n)]
    for opt in opts:
        for g in opt.param_groups:
            for p in g["params"]:
                out += [v.detach().clone() for k, v in sorted(opt.state[p].items()) if k != "step"]
    if kind == "sac":
        out.append(agent.alpha.clone())
    return out


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), i


def _to_dev(arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in arrays)


def _random_batches(kind, rows, n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *shape: torch.rand(shape, generator=g, device=DEV) * 2 - 1
    out = []
    for _ in range(n):
        batch = (rnd(rows, 10), rnd(rows, 2), torch.randn(rows, generator=g, device=DEV), rnd(rows, 10),
                 (torch.rand(rows, generator=g, device=DEV) > 0.1).float())
        noise = tuple(torch.randn((rows, 2), generator=g, device=DEV) for _ in range({"sac": 2, "td3": 1, "ddpg": 0}[kind]))
        out.append((batch, noise or None))
    return out


@pytest.fixture(scope="module", params=lr.KINDS)
def fixture(request):
    return request.param, lr.load_fixture(request.param, GOLDEN)


# ---- 1. the reference's own update_parameters ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows", lr.CASES)
def test_fixture_parity(fixture, rows):
    """K = 6 update_batch calls on the fixture's batches and noise.  Per network d(fused) <= 2 d(float32 reference), d the
    2-norm distance from the float64 restatement on the sampled indices (one-element log_alpha: floor 4 ulp); every
    recorded scalar within max(2 |reference - float64|, 1e-6 |reference|) of the reference's returned one.  td3.py returns
    nothing: there the float32 restatement's scalars (bit-equal to the reference's for SAC and DDPG,
    tests/test_learner_host.py) stand in."""
    kind, fx = fixture
    batches, noises = lr.case_inputs(fx, rows)
    agent = _learner(kind)
    for b, n in zip(batches, noises):
        agent.update_batch(*_to_dev(b), noise=_to_dev(n) or None)
    idx = {n[4:]: fx[n] for n in fx if n.startswith("idx_")}
    ratios = lr.check_networks(lr.sampled(_tensors(agent, kind), idx), fx, rows, f"{kind} fused")
    print(kind, rows, "d(fused) / d(reference-f32):", {k: round(v, 3) for k, v in ratios.items()})
    log = agent.losses().astype(np.float64)
    assert log.shape == (lr.K, 8) and int(agent._updates.item()) == lr.K
    p = f"b{rows}_"
    ref, f64 = fx[p + "scalars_ref"], fx[p + "scalars_f64"]
    if kind == "td3":
        ref = fx[p + "scalars_f32"]
    worst = 0.0
    for u in range(lr.K):
        for c in range(lr.COLUMNS):
            bound = max(2.0 * abs(ref[u, c] - f64[u, c]), 1e-6 * abs(ref[u, c]))
            err = abs(log[u, c] - ref[u, c])
            print(f"{kind} B={rows} update {u} column {c}: fused {log[u, c]:.9g} reference {ref[u, c]:.9g} float64 "
                  f"{f64[u, c]:.9g} error {err:.3e} bound {bound:.3e}")
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else math.inf))
            assert err <= bound, (u, c, err, bound)
    print(kind, rows, "worst scalar error / bound", worst)
    assert (log[:, 6:] == 0).all()
    assert list(log[:, 5]) == ([1, 0, 1, 0, 1, 0] if kind == "td3" else [1] * lr.K)
    if kind == "sac":
        # update 0 ran with alpha = 2: the critic of update 1 has seen that target.  A restatement that starts alpha at
        # exp(0) = 1 records a critic loss of update 1 outside the bound.
        _, alt = lr.run(kind, batches[:2], noises[:2], torch.float64, alpha0=1.0)
        bound = max(2.0 * abs(ref[1, 0] - f64[1, 0]), 1e-6 * abs(ref[1, 0]))
        assert abs(log[1, 0] - ref[1, 0]) <= bound
        assert abs(log[1, 0] - alt[1, 0]) > bound, (log[1, 0], alt[1, 0])
        assert log[0, 3] == 0.0 and abs(log[0, 4] - math.exp(-3e-4)) < 1e-6
    agent.close()


# ---- 2. the tail launch alone -------------------------------------------------------------------------------------------
def _ulps(got, want):
    return abs(float(got) - float(want)) / lr.ulp32(want) if want != 0 else (0.0 if got == 0 else math.inf)


class _Tail:
    """The arguments of one uavx_learner_tail call, every device value inside one NaN-filled arena."""

    def __init__(self, capacity=4):
        self.lib = _actor_lib.load()
        self.capacity = capacity
        self.arena = torch.full((256,), NAN, dtype=torch.float32, device=DEV)
        self.slots = dict(loss=(8, 3), lpm=(24, 1), la=(40, 1), m=(56, 1), v=(72, 1), alpha=(88, 1),
                          log=(104, capacity * 8))
        self.counts = torch.zeros(2, dtype=torch.int64, device=DEV)          # Adam step, updates
        self.losses = (ctypes.c_void_p * 3)()

    def view(self, name):
        o, n = self.slots[name]
        return self.arena[o:o + n]

    def guards_intact(self):
        keep = torch.ones(256, dtype=torch.bool, device=DEV)
        for o, n in self.slots.values():
            keep[o:o + n] = False
        return bool(torch.isnan(self.arena[keep]).all())

    def call(self, kind=_actor_lib.SAC, alpha_step=True, te=-2.0, lr_=3e-4, actor_updated=1, capacity=None, log=True,
             alpha=True):
        ptr = lambda name: self.view(name).data_ptr()
        for i in range(3):
            self.losses[i] = ptr("loss") + 4 * i
        step = (ptr("lpm"), te, ptr("la"), ptr("m"), ptr("v"), self.counts.data_ptr(), lr_, 0.9, 0.999, 1e-8)
        none = (None, 0.0, None, None, None, None, 0.0, 0.0, 0.0, 0.0)
        return self.lib.uavx_learner_tail(kind, self.losses, *(step if alpha_step else none), ptr("alpha") if alpha else None,
                                          ptr("log") if log else None, self.capacity if capacity is None else capacity,
                                          self.counts[1:].data_ptr(), actor_updated, None)


@pytest.mark.parametrize("count", [0, 1, 999])
@pytest.mark.parametrize("lpm", [-3.0, 0.0, 2.5, 2.0])
def test_tail_alone_against_float64(lpm, count):
    """log_alpha, m, v, alpha and alpha_loss within 4 ulp of include/uavx_learner.h's formulas in float64
    (tests/learner_ref.py alpha_step); lpm = 2.0 is exactly -target_entropy: h = 0.  A property of the arithmetic, shared
    with uavx_optim.h: the float32 form m + (g - m)(1 - beta1) is a few ulp of its OPERANDS from float64, so where the sum
    cancels (m = 0.05, g = -0.5 gives a tenth of its terms) it is 7.2 ulp of its result away, in the kernel as in numpy
    float32 and torch's float32 Adam.  The 4-ulp statement is for states without that cancellation: the moments here are
    small against every nonzero g."""
    f32 = lambda x: float(np.float32(x))
    la0, m0, v0 = (f32(0.3), 0.0, 0.0) if count == 0 else (f32(-0.2), f32(5e-4), f32(2e-5))
    t = _Tail()
    t.view("loss").copy_(torch.tensor([1.5, 2.5, -0.75]))
    t.view("lpm").fill_(lpm)
    t.view("la").fill_(la0)
    t.view("m").fill_(m0)
    t.view("v").fill_(v0)
    t.view("alpha").fill_(2.0)
    t.view("log").fill_(7.0)
    t.counts.copy_(torch.tensor([count, 1]))
    assert t.call() == _actor_lib.OK
    torch.cuda.synchronize()
    loss, la, m, v, alpha = lr.alpha_step(la0, m0, v0, count + 1, lpm - 2.0)
    got = {k: float(t.view(k)) for k in ("la", "m", "v", "alpha")}
    row = t.view("log").view(4, 8)[1].tolist()                 # updates was 1: row 1
    for name, g, w in (("log_alpha", got["la"], la), ("m", got["m"], m), ("v", got["v"], v), ("alpha", got["alpha"], alpha),
                       ("alpha_loss", row[3], loss)):
        print(f"lpm {lpm} count {count} {name}: got {g!r} float64 {float(w)!r} ulps {_ulps(g, w):.2f}")
        assert _ulps(g, w) <= 4.0, name
    assert row == [1.5, 2.5, -0.75, row[3], got["alpha"], 1.0, 0.0, 0.0]
    assert t.counts.tolist() == [count + 1, 2]
    others = t.view("log").view(4, 8)[[0, 2, 3]]
    assert bool((others == 7.0).all())                          # one row is written
    assert t.guards_intact()
    if lpm == 2.0 and count == 0:
        assert got["la"] == la0 and got["m"] == 0.0 and got["v"] == 0.0         # h = 0: nothing moves


def test_tail_ring_wraps_and_null_log_alpha_writes_only_the_row():
    t = _Tail(capacity=4)
    for name, x in (("lpm", 0.5), ("la", -0.1), ("m", 0.01), ("v", 0.001), ("alpha", 0.7)):
        t.view(name).fill_(x)
    t.view("log").fill_(NAN)
    before = t.arena.clone()
    for u in range(6):
        t.view("loss").copy_(torch.tensor([10.0 + u, 20.0 + u, 30.0 + u]))
        kind = (_actor_lib.TD3, _actor_lib.DDPG)[u % 2]
        assert t.call(kind=kind, alpha_step=False, actor_updated=u % 2, alpha=u < 4) == _actor_lib.OK
    torch.cuda.synchronize()
    assert t.counts.tolist() == [0, 6]                          # the Adam count is not the tail's without log_alpha
    log = t.view("log").view(4, 8).cpu().numpy()
    for u in (2, 3, 4, 5):                                      # rows 0, 1 were overwritten by updates 4, 5
        want = [10.0 + u, 0.0 if u % 2 else 20.0 + u, 30.0 + u if u % 2 else 0.0, 0.0, 0.7 if u < 4 else 0.0, u % 2, 0.0,
                0.0]
        assert log[u % 4].tolist() == pytest.approx(want, abs=0, rel=1e-7), u
    for name in ("lpm", "la", "m", "v", "alpha"):
        assert torch.equal(t.view(name), before[t.slots[name][0]:t.slots[name][0] + 1]), name
    assert t.guards_intact()


def test_tail_rejected_arguments_enqueue_nothing():
    t = _Tail()
    for name, x in (("loss", 1.0), ("lpm", 0.5), ("la", -0.1), ("m", 0.01), ("v", 0.001), ("alpha", 0.7), ("log", 3.0)):
        t.view(name).fill_(x)
    t.counts.copy_(torch.tensor([5, 2]))
    before = t.arena.clone()
    bad = _actor_lib.ERR_INVALID_ARG
    assert t.call(capacity=0) == bad
    assert t.call(log=False) == bad
    assert t.call(lr_=-1e-3) == bad
    assert t.call(kind=_actor_lib.TD3) == bad                   # an alpha step for a learner that has none
    assert t.call(alpha=False) == bad
    assert t.call(actor_updated=2) == bad
    torch.cuda.synchronize()
    assert t.counts.tolist() == [5, 2]
    assert torch.equal(t.arena.view(torch.int32), before.view(torch.int32))


# ---- 3. the update is its pieces ------------------------------------------------------------------------------------------
def _hand_composed(kind, work):
    """The same six updates from the public classes of §13-§18, in the reference's order; returns the modules."""
    from gym_uav_collision_avoidance_amd.fused_critic import FusedCriticLoss, FusedTarget
    from gym_uav_collision_avoidance_amd.fused_optim import FusedAdam, soft_update
    from gym_uav_collision_avoidance_amd.fused_policy_grad import FusedPolicyGrad
    nets = lr.networks(kind, device=DEV)
    critic, critic_t = nets["critic"], nets["critic_target"]
    actor = nets["policy" if kind == "sac" else "actor"]
    closs, pg = FusedCriticLoss(critic), FusedPolicyGrad(actor, critic)
    tau = 5e-3
    if kind == "sac":
        target = FusedTarget(actor, critic_t)
        copt = FusedAdam(torch.optim.Adam(critic.parameters(), lr=3e-4))
        aopt = FusedAdam(torch.optim.Adam(actor.parameters(), lr=3e-4))
        for (s, a, r, s2, m), (n0, n1) in work:
            y = target(s2, r, m, alpha=2.0, noise=n0)
            closs.backward(s, a, y)
            copt.step()
            pg.backward(s, alpha=2.0, noise=n1)
            aopt.step()
            soft_update(critic_t, critic, tau)                  # sac.py:95-96, after the policy step
            target.refresh()
        return nets
    actor_t = nets["actor_target"]
    amsgrad = kind == "ddpg"
    target = FusedTarget(actor_t, critic_t)
    copt = FusedAdam(torch.optim.Adam(critic.parameters(), lr=1e-3 if amsgrad else 3e-4, amsgrad=amsgrad))
    aopt = FusedAdam(torch.optim.Adam(actor.parameters(), lr=1e-4 if amsgrad else 3e-4, amsgrad=amsgrad), target=actor_t,
                     tau=tau)
    for u, ((s, a, r, s2, m), noise) in enumerate(work):
        y = target(s2, r, m, noise=noise[0]) if kind == "td3" else target(s2, r, m)
        closs.backward(s, a, y)
        copt.step(update_target=False)
        if kind == "ddpg" or u % 2 == 0:
            pg.backward(s)
            aopt.step(update_target=True)
            soft_update(critic_t, critic, tau)
            target.refresh()
    return nets


@pytest.mark.parametrize("rows", [17, 256])
@pytest.mark.parametrize("kind", lr.KINDS)
def test_update_equals_the_hand_composed_launches(kind, rows):
    work = _random_batches(kind, rows, 6, seed=300 + rows)
    kw = dict(automatic_entropy_tuning=False) if kind == "sac" else {}
    agent = _learner(kind, **kw)
    for batch, noise in work:
        agent.update_batch(*batch, noise=noise)
    nets = _hand_composed(kind, work)
    torch.cuda.synchronize()
    for name in NETS[kind]:
        for (n, p), q in zip(getattr(agent, name).named_parameters(), nets[name].parameters()):
            assert torch.equal(p.view(torch.int32), q.view(torch.int32)), (name, n)
    log = agent.losses()
    if kind == "sac":
        assert (log[:, 3] == 0).all() and (log[:, 4] == 2.0).all() and float(agent.alpha) == 2.0     # alpha stays `alpah`
    agent.close()


# ---- 4. graph replay ------------------------------------------------------------------------------------------------------
E, N, T = 16, 4, 32


def _memory(seed=3):
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    env = BatchedMultiUAVWorld2D(E, num_agents=N, device=DEV, seed=seed)
    mem = DeviceReplay(env, horizon=T)
    mem.begin(env.reset())
    g = torch.Generator(device=DEV).manual_seed(100 + seed)
    for _ in range(T + 3):
        mem.action_slot().copy_(torch.rand((E, N, 2), generator=g, device=DEV) * 2 - 1)
        mem.step(polar=True, auto_reset="agent0_done", step_cap=12)
    return env, mem


@pytest.fixture(scope="module")
def memory():
    env, mem = _memory()
    yield mem
    env.close()


@pytest.mark.parametrize("own_generator", [True, False])
@pytest.mark.parametrize("kind,kw", [("sac", {}), ("td3", {}), ("ddpg", {}), ("sac", {"target_update_interval": 2})],
                         ids=["sac", "td3", "ddpg", "sac-interval2"])
def test_graph_replay_equals_eager_updates(kind, kw, own_generator, memory):
    def gen(seed):
        if own_generator:
            return torch.Generator(device=DEV).manual_seed(seed)
        torch.cuda.manual_seed(seed)
        return None

    eager = _learner(kind, generator=gen(77), **kw)
    for _ in range(6):
        eager.update_parameters(memory, 256)
    torch.cuda.synchronize()
    want, want_log = _state(eager, kind), eager.losses()
    graphed = _learner(kind, generator=gen(77), memory=memory, **kw)
    before = _state(graphed, kind)
    graphed.capture(256)
    torch.cuda.synchronize()
    _same(_state(graphed, kind), before)                        # the capture itself ran nothing
    assert len(graphed._graphs) == (2 if kind == "td3" or kw else 1)          # full and critic-only / no-target graphs
    graphed.run(6)
    torch.cuda.synchronize()
    _same(_state(graphed, kind), want)
    got_log = graphed.losses()
    assert got_log.shape == (6, 8) and np.array_equal(got_log.view(np.int32), want_log.view(np.int32))
    assert int(graphed._updates.item()) == int(eager._updates.item()) == 6 == graphed.updates
    if kind == "td3":
        assert list(got_log[:, 5]) == [1, 0, 1, 0, 1, 0]
    obs = memory.state                                          # [E, N, 10]: select_action follows replayed actor steps
    assert torch.equal(graphed.select_action(obs, evaluate=True), eager.select_action(obs, evaluate=True))
    for a in (eager, graphed):
        a.close()


def test_update_during_capture_needs_reserve():
    agent = _learner("td3")
    (batch, noise), = _random_batches("td3", 64, 1, seed=5)
    agent.update_batch(*batch, noise=noise)                     # the kernels are loaded
    fresh = _learner("td3")
    scratch = torch.zeros(8, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="reserve"):
        with torch.cuda.graph(g):
            scratch.add_(1)
            fresh.update_batch(*batch, noise=noise)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="capture"):
        fresh.run(1)
    for a in (agent, fresh):
        a.close()


@pytest.mark.parametrize("kind", lr.KINDS)
def test_select_action_follows_the_actor_steps(kind):
    agent = _learner(kind)
    live = agent.policy if kind == "sac" else agent.actor
    obs = torch.rand((5, 4, 10), generator=torch.Generator(device=DEV).manual_seed(9), device=DEV) * 2 - 1
    seen = []
    for batch, noise in [(None, None)] + _random_batches(kind, 32, 3, seed=600):
        if batch is not None:
            agent.update_batch(*batch, noise=noise)
        got = agent.select_action(obs, evaluate=True)
        with torch.no_grad():
            want = live.act(obs, evaluate=True)
        assert got.shape == (5, 4, 2) and float((got - want).abs().max()) <= 1e-5
        seen.append(got.clone())
    moved = [not torch.equal(a, b) for a, b in zip(seen, seen[1:])]
    assert moved == ([True, False, True] if kind == "td3" else [True] * 3)      # TD3's update 1 leaves the actor alone
    agent.close()


# ---- 5. checkpoints -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", lr.KINDS)
def test_checkpoint_continues_bit_for_bit(kind, tmp_path):
    from gym_uav_collision_avoidance_amd import policy
    work = _random_batches(kind, 32, 6, seed=400)
    whole = _learner(kind)
    for i, (batch, noise) in enumerate(work):
        if i == 3:
            where = whole.save_checkpoint(str(tmp_path))
        whole.update_batch(*batch, noise=noise)
    resumed = _cls(kind)(device=DEV)
    resumed.load_checkpoint(str(tmp_path))
    assert resumed.updates == 3 and int(resumed._updates.item()) == 3
    for batch, noise in work[3:]:
        resumed.update_batch(*batch, noise=noise)
    torch.cuda.synchronize()
    _same(_state(resumed, kind), _state(whole, kind))
    assert np.array_equal(resumed.losses(last=3).view(np.int32), whole.losses(last=3).view(np.int32))
    # the file is the reference's: policy.py's loaders read it
    path = str(tmp_path) if kind == "ddpg" else where
    mid = _learner(kind)
    for batch, noise in work[:3]:
        mid.update_batch(*batch, noise=noise)
    actor = policy.load_actor(path, device=DEV)
    live = mid.policy if kind == "sac" else mid.actor
    for p, q in zip(actor.parameters(), live.parameters()):
        assert torch.equal(p, q)
    for target in (False, True):
        crit = policy.load_critic(path, target=target, device=DEV)
        for p, q in zip(crit.parameters(), (mid.critic_target if target else mid.critic).parameters()):
            assert torch.equal(p, q)
    assert not torch.equal(next(mid.critic.parameters()), next(mid.critic_target.parameters()))
    for a in (whole, resumed, mid):
        a.close()


# ---- 6. SAC's delayed target update ---------------------------------------------------------------------------------------
def test_sac_target_update_interval():
    agent = _learner("sac", target_update_interval=2)
    work = _random_batches("sac", 32, 4, seed=500)
    (s, a, *_), _ = work[0]
    flat = lambda: torch.cat([p.detach().reshape(-1) for p in agent.critic_target.parameters()]).clone()
    packed = lambda: torch.cat(agent._target_h.q(s, a), dim=1).clone()
    t_prev, q_prev = flat(), packed()
    for u, (batch, noise) in enumerate(work):
        agent.update_batch(*batch, noise=noise)
        t_now, q_now = flat(), packed()
        if u % 2 == 0:
            assert not torch.equal(t_now, t_prev) and not torch.equal(q_now, q_prev), u
            with torch.no_grad():                               # the packed handle is the new target
                ref = torch.cat(agent.critic_target(s, a), dim=1)
            assert float((q_now - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
        else:
            assert torch.equal(t_now, t_prev) and torch.equal(q_now, q_prev), u
        t_prev, q_prev = t_now, q_now
    agent.close()

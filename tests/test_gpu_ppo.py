"""PPO on the device ring (ppo.py) on the MI355X, 64 envs x 2 agents, T = 8: two learners built from the same
seeds are byte-equal after two rollouts and updates; the advantages an update used are gae_ref's on the ring it saw; the
probability ratio over the first minibatch of the first epoch is exactly 1; a learner saved after an update and loaded into a
fresh one continues to the same bytes.  What an update computes is held to tests/ppo_ref.py, a float64 restatement on the CPU:
on a crafted ring of 32 x 3 (768 rows, both kinds of zero weight, ratios on both sides of the clip interval at both signs of
the advantage) the weight exactly and the three losses and every parameter's gradient, unclipped and clipped, within four
times what float32 arithmetic alone costs; act() stores u, tanh(u) and log π(u); on a live ring the weight is what a forward
simulation of every agent from the steps' returned dones and flags says.  No test asserts that a policy learns, and none
should: these pin what is computed, not what comes of it."""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import gae_layouts
import gae_ref
import ppo_ref
from gae_ref import same

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
E, N, T = 64, 2, 8
STEP = dict(polar=True, auto_reset="agent0_done", step_cap=5)


def _build(torch_seed=0):
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.ppo import PPO
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    torch.manual_seed(torch_seed)
    env = BatchedMultiUAVWorld2D(E, num_agents=N, device=DEV, seed=5)
    mem = DeviceReplay(env, horizon=T)
    mem.begin(env.reset())
    gen = torch.Generator(device=DEV).manual_seed(7)
    return env, mem, gen, PPO(mem, generator=gen, epochs=2, minibatches=4)


def _iterate(mem, ppo):
    for _ in range(T):
        ppo.act()
        mem.step(**STEP)
    return ppo.update()


def _state(mem, ppo):
    """Everything a continued run depends on, as CPU tensors."""
    out = [p.detach().cpu().clone() for p in ppo.params] + [ppo.u.cpu().clone(), ppo.logp.cpu().clone()]
    out += [mem.obs.cpu().clone(), mem.rew.cpu().clone(), mem.done.cpu().clone()]
    for st in ppo.optimizer.state_dict()["state"].values():
        out += [st["exp_avg"].cpu().clone(), st["exp_avg_sq"].cpu().clone(), st["step"].cpu().clone()]
    return out


@functools.lru_cache(maxsize=None)
def _run(tag):
    """Two rollouts and updates; what the first update saw and used, a run file written after it, and the final state."""
    from gym_uav_collision_avoidance_amd.checkpoint import save_run
    env, mem, gen, ppo = _build()
    losses = _iterate(mem, ppo)
    seen = dict(count=mem.count, rew=mem.rew.cpu().numpy(), done=mem.done.cpu().numpy(), skip=mem.skip.cpu().numpy(),
                ended=mem.ended.cpu().numpy(), values=ppo.values.cpu().numpy(), ratio=ppo.first_ratio.cpu().numpy(),
                out=[t.cpu().numpy() for t in ppo.advantages.outputs], stats=[float(x) for x in ppo.advantages.stats],
                losses={k: v for k, v in losses.items()})
    folder = tempfile.mkdtemp(prefix="uavx_ppo_")
    atexit.register(shutil.rmtree, folder, True)
    path = os.path.join(folder, "run.pt")
    save_run(path, env=env, memory=mem, agent=ppo, generator=gen, extra={"t": mem.count})
    _iterate(mem, ppo)
    final = _state(mem, ppo)
    env.close()
    return seen, path, final


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8))
                                    for x, y in zip(a, b))


def test_two_learners_from_the_same_seeds_are_byte_equal():
    (_, _, a), (_, _, b) = _run("a"), _run("b")
    assert _equal(a, b)
    assert all(bool(torch.isfinite(x.float()).all()) for x in a)


def test_the_update_used_the_reference_advantages_of_the_ring_it_saw():
    seen, _, _ = _run("a")
    assert seen["count"] == T
    kw = dict(rew=seen["rew"], done=seen["done"], values=seen["values"], count=seen["count"], steps=T, gamma=0.99, lam=0.95,
              learners=N, skip=seen["skip"], ended=seen["ended"])
    adv, ret, valid = gae_ref.gae(**kw)
    norm, (n, mean, std) = gae_ref.normalise(adv, valid, seen["count"], T)
    slots = gae_ref.window_slots(seen["count"], T, T + 1)
    for got, want in zip(seen["out"], (adv, ret, valid, norm)):
        assert same(got[slots], want[slots])
    assert seen["stats"][0] == n and same(np.float64(seen["stats"][1:]), np.float64([mean, std]))
    assert 0 < n < T * E * N and seen["skip"].any()                          # resets are in the rollout
    for k, v in seen["losses"].items():
        assert v.dim() == 0 and v.device.type == "cuda" and bool(torch.isfinite(v)), k


def test_the_first_minibatch_of_the_first_epoch_has_ratio_one():
    seen, _, _ = _run("a")
    ratio = seen["ratio"]
    print("first minibatch: ratio min", ratio.min(), "max", ratio.max(), "rows != 1:", int((ratio != 1.0).sum()), "of", ratio.size)
    assert ratio.shape == (T * E * N // 4,) and np.all(ratio == np.float32(1.0))


# ---- what an update computes: one full-batch step against tests/ppo_ref.py in float64 ------------------------------------------

UPDATE = dict(ent_coef=0.01)
QUANTITIES = ("policy_loss", "value_loss", "entropy")
ROW_ORDERS = 8


def _crafted_learner(max_grad_norm=None):
    """A PPO on gae_layouts.ppo_ring() (32 x 3, T = 12, two learners, count = 17: 768 rows) with seeded obs in [-1, 1], seeded
    N(0, 1) pre-squash samples in every slot and log π_old = the policy's own float64 log density of them plus a seeded offset
    in ±0.6, moved by 0.01 wherever the ratio would come within 2e-3 of a clip edge."""
    from gym_uav_collision_avoidance_amd.ppo import PPO
    mem = gae_layouts.CraftedRing(gae_layouts.ppo_ring(), DEV)
    g = torch.Generator().manual_seed(31)
    mem.obs.copy_(torch.rand(mem.obs.shape, generator=g) * 2 - 1)
    torch.manual_seed(8)
    ppo = PPO(mem, generator=torch.Generator(device=DEV).manual_seed(9), epochs=1, minibatches=1, max_grad_norm=max_grad_norm,
              **UPDATE)
    ppo.u.copy_(torch.randn(ppo.u.shape, generator=g))
    policy, _ = ppo_ref.networks(ppo, torch.float64)
    with torch.no_grad():
        mean, log_std = policy(mem.obs.cpu().double())
        logp, _ = ppo_ref.log_density(mean, log_std, ppo.u.cpu().double())
    offset = torch.rand(logp.shape, generator=g, dtype=torch.float64) * 1.2 - 0.6
    for _ in range(2):
        old = (logp + offset).to(torch.float32)
        ratio = torch.exp(logp - old.double())
        near = ((ratio - 0.8).abs() < 2e-3) | ((ratio - 1.2).abs() < 2e-3)
        offset = torch.where(near, offset + 0.01, offset)
    ppo.logp.copy_(old)
    return mem, ppo


@functools.lru_cache(maxsize=None)
def _crafted_update(max_grad_norm):
    """(float64 restatement, float32 restatement, what PPO.update() on the GPU left) of the same step."""
    mem, ppo = _crafted_learner(max_grad_norm)
    b = ppo_ref.batch(mem, ppo, mem.T)
    kw = dict(max_grad_norm=max_grad_norm, **UPDATE)
    ref64 = ppo_ref.update(b, *ppo_ref.networks(ppo, torch.float64), torch.float64, **kw)
    g = torch.Generator().manual_seed(32)
    orders = [None] + [torch.randperm(ref64["weight"].size, generator=g) for _ in range(ROW_ORDERS - 1)]
    ref32 = [ppo_ref.update(b, *ppo_ref.networks(ppo, torch.float32), torch.float32, order=o, **kw) for o in orders]
    names = [f"policy.{n}" for n, _ in ppo.policy.named_parameters()] + [f"value.{n}" for n, _ in ppo.value.named_parameters()]
    losses = ppo.update()
    got = dict(weight=ppo.weight.cpu().numpy(), grads=[p.grad.detach().cpu() for p in ppo.params],
               **{k: losses[k].cpu() for k in QUANTITIES})
    return ref64, ref32, got, names


@pytest.mark.parametrize("max_grad_norm", [None, 0.5], ids=["unclipped", "clip_0.5"])
def test_one_full_batch_update_against_the_float64_restatement(max_grad_norm):
    """Weight exactly; the three losses and every parameter's gradient within 4 · e32 of the float64 restatement, e32 being the
    distance of the same restatement in float32 on the CPU from it (max |Δ| over the tensor / max |float64|): the GPU's
    and the CPU's float32 evaluations are the same graph and differ in summation order and GEMM blocking only, while a wrong
    mask, sign, clip side or denominator moves a gradient by order 1.  For a quantity of ONE element (the three losses and the
    value head's bias gradient) one float32 evaluation is one draw of a rounding error and is now and then a tenth of its
    usual size (8e-9 for that bias, a seventh of a float32 half-ulp), which no other float32 evaluation can match within 4x,
    the CPU's own in another row order included: there e32 is the largest distance over the float32 evaluations in eight row
    orders (the rows as they lie and seven seeded permutations; PPO itself draws one).  Tensors use the one evaluation.
    Measured on the MI355X: e32 7e-8 ... 1.1e-6, the GPU at 0.2 ... 2.1 of e32 except value.linear2.weight at 3.40 (unclipped)
    and 3.85 (clipped); all figures in DESIGN.md §28."""
    ref64, ref32, got, names = _crafted_update(max_grad_norm)
    # the inputs reach what the test is about
    w, ratio, adv = ref64["weight"], ref64["ratio"].numpy(), ref64["adv"].numpy()
    assert w.shape == (768,) and np.array_equal(got["weight"], w)
    c = gae_layouts.ppo_ring()
    _, why = ppo_ref.weight_loop(c["done"], c["skip"], c["ended"], 17, 12, 2)
    assert (why == 2).sum() > 0 and (why == 3).sum() > 0 and (why == 4).sum() > 0 and (why == 5).sum() > 0
    live = w > 0
    assert 0.5 * w.size < live.sum() < w.size
    for sign in (adv > 0, adv < 0):
        for side in (ratio < 0.8, ratio > 1.2):
            share = (live & sign & side).sum() / live.sum()
            assert share >= 0.05, share
    assert np.abs(ratio[live] - 0.8).min() > 1e-3 and np.abs(ratio[live] - 1.2).min() > 1e-3
    if max_grad_norm is not None:
        assert ref64["norm"] > 1.0, ref64["norm"]
    failed = []
    rows = [(q, ref64[q], [r[q] for r in ref32], got[q]) for q in QUANTITIES]
    rows += [(n, ref64["grads"][j], [r["grads"][j] for r in ref32], got["grads"][j]) for j, n in enumerate(names)]
    for name, g64, g32, gg in rows:
        single = g64.numel() == 1
        e32 = max(ppo_ref.distance(x, g64) for x in (g32 if single else g32[:1]))
        d = ppo_ref.distance(gg, g64)
        print(f"{name:28s} e32 = {e32:.3e}{' (of %d row orders)' % ROW_ORDERS if single else ''}   gpu = {d:.3e}   gpu / e32 = {d / e32:.2f}")
        if not d <= 4.0 * e32:
            failed.append((name, e32, d))
    assert not failed, failed


def test_act_stores_the_sample_its_squash_and_its_log_density():
    """act() on the crafted ring: the action slot is tanh of the stored pre-squash sample bit for bit, and the stored log π is
    the float64 log density of that sample under float64 copies of the policy, within 2^-19 · Σ|terms| (test_ppo_host.py)
    plus four times what the float32 network outputs' distance from float64, measured on the CPU, moves the density by:
    |∂ log π / ∂μ| = |z| / σ and |∂ log π / ∂ log σ| = |z² − 1| per action dimension."""
    mem, ppo = _crafted_learner()
    s = mem.count % mem.L
    before_u, before_logp = ppo.u.clone(), ppo.logp.clone()
    out = ppo.act()
    assert out.data_ptr() == mem.action_slot().data_ptr()
    u = ppo.u[s]
    assert torch.equal(out.view(torch.int32), torch.tanh(u).view(torch.int32)) and float(out.abs().max()) <= 1.0
    others = [k for k in range(mem.L) if k != s]
    assert torch.equal(ppo.u[others], before_u[others]) and torch.equal(ppo.logp[others], before_logp[others])
    assert not torch.equal(u, before_u[s]) and float(u.std()) > 0.5           # a fresh sample went into the slot
    obs = mem.state.cpu()
    with torch.no_grad():
        p64, _ = ppo_ref.networks(ppo, torch.float64)
        p32, _ = ppo_ref.networks(ppo, torch.float32)
        mean, log_std = p64(obs.double())
        mean32, log_std32 = p32(obs)
        gmean, glog_std = (t.cpu() for t in ppo.policy(mem.state))
    want, scale = ppo_ref.log_density(mean, log_std, u.cpu().double())
    e_mean, e_log_std = float((mean32.double() - mean).abs().max()), float((log_std32.double() - log_std).abs().max())
    z = (u.cpu().double() - mean) / log_std.exp()
    moved = (z.abs() / log_std.exp() * e_mean + (z * z - 1).abs() * e_log_std).sum(-1)
    tol = 2.0 ** -19 * scale + 4.0 * moved
    err = (ppo.logp[s].cpu().double() - want).abs()
    print(f"act: network outputs e32 mean {ppo_ref.distance(mean32, mean):.3e} log_std {ppo_ref.distance(log_std32, log_std):.3e}; "
          f"gpu mean {ppo_ref.distance(gmean, mean):.3e} log_std {ppo_ref.distance(glog_std, log_std):.3e}; "
          f"log pi worst |gpu - float64| / tolerance = {float((err / tol).max()):.3f}, worst |gpu - float64| = {float(err.max()):.3e}")
    assert bool((err <= tol).all())
    # the sample is the policy's: (u − μ) / σ is standard normal over the slot's 192 draws
    assert abs(float(z.mean())) < 0.3 and 0.7 < float(z.std()) < 1.3


@pytest.mark.parametrize("packed_flags", [False, True], ids=["rows", "packed"])
def test_weight_on_a_live_ring_against_what_the_steps_returned(packed_flags):
    """64 x 2, T = 8, step_cap = 3, auto_reset = "agent0_done", 20 steps.  Each step's returned done row and flags go to the host
    in step order; every agent is then simulated forward from those lists alone (a sample while alive; parked after its own
    done until its env's episode ends or the env is re-initialised), and the update's weight over the last 8 steps must be
    that simulation's."""
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.ppo import PPO
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    E_, N_, T_, steps = 64, 2, 8, 20
    # a world of 2 x 2: a UAV covers up to 0.2 per step, so within the three steps of an episode some leave it (done) while
    # agent 0 of their env does not -- in the default 50 x 50 world no agent is ever done before the step cap
    env = BatchedMultiUAVWorld2D(E_, num_agents=N_, device=DEV, seed=11, x_size=2.0, y_size=2.0, collider_radius=0.1)
    mem = DeviceReplay(env, horizon=T_, packed_flags=packed_flags)
    mem.begin(env.reset())
    torch.manual_seed(3)
    ppo = PPO(mem, generator=torch.Generator(device=DEV).manual_seed(12), epochs=1, rollout=T_)
    history = []
    for _ in range(steps):
        ppo.act()
        _, _, done, info = mem.step(polar=True, auto_reset="agent0_done", step_cap=3)
        d = done.cpu().numpy().astype(np.uint8)
        if packed_flags:
            history.append((d & 1, (d[:, 0] & 2) != 0, (d[:, 0] & 4) != 0))
        else:
            history.append((d & 1, info["reset_mask"].cpu().numpy().copy(), info["ended"].cpu().numpy().copy()))
    ppo.update()
    sample = np.zeros((steps, E_, N_), np.float32)
    parked_rows = reinit_rows = 0
    for e in range(E_):
        parked = [False] * N_
        for t, (done_row, reinit, ended) in enumerate(history):
            if reinit[e]:
                parked = [False] * N_
                reinit_rows += 1
                continue
            for i in range(N_):
                if parked[i]:
                    parked_rows += t >= steps - T_
                else:
                    sample[t, e, i] = 1.0
                    parked[i] = bool(done_row[e, i])
            if ended[e]:
                parked = [False] * N_
    want = sample[-T_:].reshape(-1)
    got = ppo.weight.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    n = int(ppo.advantages.stats.n)
    print(f"in the window: {parked_rows} parked rows, {int(want.sum())} samples, n = {n}; re-initialisation rows: {reinit_rows}")
    assert parked_rows > 0 and reinit_rows > 0 and 0 < want.sum() <= n < want.size
    assert want.sum() + parked_rows == n                                     # parked rows are valid rows that are no samples
    env.close()


def test_a_saved_learner_continues_to_the_same_bytes():
    from gym_uav_collision_avoidance_amd.checkpoint import load_run
    _, path, final = _run("a")
    env, mem, gen, ppo = _build(torch_seed=99)                               # other initial weights: the file must bring them
    gen.manual_seed(1234)
    extra = load_run(path, env=env, memory=mem, agent=ppo, generator=gen)
    assert extra == {"t": T} and mem.count == T and ppo.updates == 1
    _iterate(mem, ppo)
    assert _equal(_state(mem, ppo), final)
    env.close()

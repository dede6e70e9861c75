"""PPO(fused_heads=True) on the MI355X (ppo.py, ppo_heads.py): the learner whose sampling and losses run in
HIP between torch's GEMMs, held to what test_gpu_ppo.py holds the torch learner to.  The crafted full-batch update on
gae_layouts.ppo_ring (768 rows, both kinds of zero weight, ratios on both sides of the clip interval at both signs of the
advantage): the weight exactly, the three losses and every parameter's gradient, unclipped and clipped, within four times
what float32 arithmetic alone costs of tests/ppo_ref.py in float64.  On a live ring of 64 x 2, T = 8: two fused learners from
the same seeds are byte-equal after two rollouts and updates, the ratio over the first minibatch is exactly 1, a saved run
loaded into a fresh fused learner continues to the same bytes, act() writes its slot only, and a fused and a torch learner
draw from the generator alike."""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import gae_layouts
import ppo_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
E, N, T = 64, 2, 8
STEP = dict(polar=True, auto_reset="agent0_done", step_cap=5)
UPDATE = dict(ent_coef=0.01)
QUANTITIES = ("policy_loss", "value_loss", "entropy")
ROW_ORDERS = 8


# ---- one full-batch step against tests/ppo_ref.py in float64 -------------------------------------------------------------------

def _crafted_learner(max_grad_norm=None, fused_heads=True):
    """A PPO on gae_layouts.ppo_ring() (32 x 3, T = 12, two learners, count = 17: 768 rows) with seeded obs in [-1, 1], seeded
    N(0, 1) pre-squash samples in every slot and log π_old = the policy's own float64 log density of them plus a seeded offset
    in ±0.6, moved by 0.01 wherever the ratio would come within 2e-3 of a clip edge."""
    from gym_uav_collision_avoidance_amd.ppo import PPO
    mem = gae_layouts.CraftedRing(gae_layouts.ppo_ring(), DEV)
    g = torch.Generator().manual_seed(31)
    mem.obs.copy_(torch.rand(mem.obs.shape, generator=g) * 2 - 1)
    torch.manual_seed(8)
    ppo = PPO(mem, generator=torch.Generator(device=DEV).manual_seed(9), epochs=1, minibatches=1, max_grad_norm=max_grad_norm,
              fused_heads=fused_heads, **UPDATE)
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
    """(float64 restatement, float32 restatement in eight row orders, what the fused update left) of the same step."""
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
               ratio=ppo.first_ratio.cpu(), **{k: losses[k].cpu() for k in QUANTITIES})
    return ref64, ref32, got, names


@pytest.mark.parametrize("max_grad_norm", [None, 0.5], ids=["unclipped", "clip_0.5"])
def test_one_fused_full_batch_update_against_the_float64_restatement(max_grad_norm):
    """Weight exactly; the three losses and every parameter's gradient within 4 · e32 of the float64 restatement, e32 as in
    test_gpu_ppo.py: the distance of the restatement in float32 on the CPU from float64, for quantities of one element the
    largest over eight row orders."""
    from gym_uav_collision_avoidance_amd import _ppo_lib
    ref64, ref32, got, names = _crafted_update(max_grad_norm)
    assert _ppo_lib.loaded()
    w, ratio, adv = ref64["weight"], ref64["ratio"].numpy(), ref64["adv"].numpy()
    assert w.shape == (768,) and np.array_equal(got["weight"], w)
    live = w > 0
    assert 0.5 * w.size < live.sum() < w.size
    for sign in (adv > 0, adv < 0):
        for side in (ratio < 0.8, ratio > 1.2):
            assert (live & sign & side).sum() / live.sum() >= 0.05
    assert np.abs(ratio[live] - 0.8).min() > 1e-3 and np.abs(ratio[live] - 1.2).min() > 1e-3
    if max_grad_norm is not None:
        assert ref64["norm"] > 1.0, ref64["norm"]
    assert got["ratio"].shape == (768,)
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


def test_act_writes_its_slot_only_and_draws_like_the_torch_learner():
    mem, ppo = _crafted_learner()
    mem2, plain = _crafted_learner(fused_heads=False)
    assert plain.heads is None and torch.equal(ppo.generator.get_state(), plain.generator.get_state())
    s = mem.count % mem.L
    before_u, before_logp = ppo.u.clone(), ppo.logp.clone()
    out = ppo.act()
    out2 = plain.act()
    assert torch.equal(ppo.generator.get_state(), plain.generator.get_state())
    assert not torch.equal(ppo.generator.get_state(), torch.Generator(device=DEV).manual_seed(9).get_state())
    assert out.data_ptr() == mem.action_slot().data_ptr() and float(out.abs().max()) <= 1.0
    others = [k for k in range(mem.L) if k != s]
    assert torch.equal(ppo.u[others], before_u[others]) and torch.equal(ppo.logp[others], before_logp[others])
    assert not torch.equal(ppo.u[s], before_u[s]) and float(ppo.u[s].std()) > 0.5
    # the same networks, the same noise: the two learners' samples agree to float32 rounding, the stored action is the
    # stored sample's tanh, the stored log π the float64 density of the stored sample (2^-19 · Σ|terms|, test_ppo_host.py)
    assert bool(((ppo.u[s] - plain.u[s]).abs() <= 2.0 ** -19 * (1.0 + plain.u[s].abs())).all())
    assert float((out - out2).abs().max()) <= 2.0 ** -19 * (1.0 + float(plain.u[s].abs().max()))
    assert float((out.double() - torch.tanh(ppo.u[s].double())).abs().max()) <= 2.0 ** -20
    with torch.no_grad():
        mean, log_std = ppo.policy(mem.state)
    want, scale = ppo_ref.log_density(mean.cpu().double(), log_std.cpu().double(), ppo.u[s].cpu().double())
    assert bool(((ppo.logp[s].cpu().double() - want).abs() <= 2.0 ** -19 * scale).all())


# ---- a live ring -----------------------------------------------------------------------------------------------------------------

def _build(torch_seed=0):
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.ppo import PPO
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    torch.manual_seed(torch_seed)
    env = BatchedMultiUAVWorld2D(E, num_agents=N, device=DEV, seed=5)
    mem = DeviceReplay(env, horizon=T)
    mem.begin(env.reset())
    gen = torch.Generator(device=DEV).manual_seed(7)
    return env, mem, gen, PPO(mem, generator=gen, epochs=2, minibatches=4, fused_heads=True)


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
    """Two rollouts and updates; what the first update left, a run file written after it, and the final state."""
    from gym_uav_collision_avoidance_amd.checkpoint import save_run
    env, mem, gen, ppo = _build()
    losses = _iterate(mem, ppo)
    seen = dict(ratio=ppo.first_ratio.cpu().numpy(), weight=ppo.weight.cpu().numpy(), losses={k: v.cpu() for k, v in losses.items()},
                kinds={k: (v.dim(), v.device.type) for k, v in losses.items()})
    folder = tempfile.mkdtemp(prefix="uavx_ppo_fused_")
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


def test_two_fused_learners_from_the_same_seeds_are_byte_equal():
    (seen, _, a), (seen2, _, b) = _run("a"), _run("b")
    assert _equal(a, b)
    assert all(bool(torch.isfinite(x.float()).all()) for x in a)
    assert set(seen["losses"]) == set(QUANTITIES)
    for k in QUANTITIES:
        assert seen["kinds"][k] == (0, "cuda") and bool(torch.isfinite(seen["losses"][k]))
        assert torch.equal(seen["losses"][k], seen2["losses"][k])
    assert 0 < seen["weight"].sum() < seen["weight"].size                    # resets are in the rollout


def test_the_first_fused_minibatch_has_ratio_one():
    seen, _, _ = _run("a")
    ratio = seen["ratio"]
    print("first minibatch: ratio min", ratio.min(), "max", ratio.max(), "rows != 1:", int((ratio != 1.0).sum()), "of", ratio.size)
    assert ratio.shape == (T * E * N // 4,) and np.all(ratio == np.float32(1.0))


def test_a_saved_fused_learner_continues_to_the_same_bytes():
    from gym_uav_collision_avoidance_amd.checkpoint import load_run
    _, path, final = _run("a")
    env, mem, gen, ppo = _build(torch_seed=99)                               # other initial weights: the file must bring them
    gen.manual_seed(1234)
    extra = load_run(path, env=env, memory=mem, agent=ppo, generator=gen)
    assert extra == {"t": T} and mem.count == T and ppo.updates == 1 and ppo.fused_heads is True
    _iterate(mem, ppo)
    assert _equal(_state(mem, ppo), final)
    env.close()

"""PPO with normalize_obs and normalize_reward (ppo.py, normalize.py) on the MI355X, in the setup of
test_gpu_ppo.py -- 64 envs x 2 agents, T = 8, two rollouts and updates -- with the torch heads and with fused_heads=True: the
first minibatch's ratio is exactly 1; the advantages the update used are gae_ref's on norm_ref's scaled rewards and the
update's own values; the record after the update is norm_ref's; two learners from the same seeds end byte-equal; a run saved
after the first update and resumed in fresh objects ends byte-equal to the run that never stopped; a learner without
normalisation refuses the saved state; select_action is the policy on the normalised observations."""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import gae_ref
import norm_ref
from gae_ref import same

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
E, N, T = 64, 2, 8
STEP = dict(polar=True, auto_reset="agent0_done", step_cap=5)
HEADS = pytest.mark.parametrize("fused", [False, True], ids=["torch_heads", "fused_heads"])


def _build(fused, torch_seed=0, normalised=True):
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.ppo import PPO
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    torch.manual_seed(torch_seed)
    env = BatchedMultiUAVWorld2D(E, num_agents=N, device=DEV, seed=5)
    mem = DeviceReplay(env, horizon=T)
    mem.begin(env.reset())
    gen = torch.Generator(device=DEV).manual_seed(7)
    ppo = PPO(mem, generator=gen, epochs=2, minibatches=4, fused_heads=fused, normalize_obs=normalised,
              normalize_reward=normalised)
    return env, mem, gen, ppo


def _iterate(mem, ppo):
    for _ in range(T):
        ppo.act()
        mem.step(**STEP)
    return ppo.update()


def _state(mem, ppo):
    """Everything a continued run depends on, as CPU tensors: test_gpu_ppo.py's, and the record, the carry and the counters."""
    out = [p.detach().cpu().clone() for p in ppo.params] + [ppo.u.cpu().clone(), ppo.logp.cpu().clone()]
    out += [mem.obs.cpu().clone(), mem.rew.cpu().clone(), mem.done.cpu().clone()]
    for st in ppo.optimizer.state_dict()["state"].values():
        out += [st["exp_avg"].cpu().clone(), st["exp_avg_sq"].cpu().clone(), st["step"].cpu().clone()]
    out += [ppo.norm._record.cpu().clone(), ppo.norm.carry.cpu().clone(),
            torch.tensor([ppo.norm.folded_obs, ppo.norm.folded_ret, mem.count, ppo.updates])]
    return out


@functools.lru_cache(maxsize=None)
def _run(fused, tag):
    """Two rollouts and updates; what the first update saw and used, a run file written after it, and the final state."""
    from gym_uav_collision_avoidance_amd.checkpoint import save_run
    env, mem, gen, ppo = _build(fused)
    empty = ppo.norm._record.cpu().numpy().view(np.uint64).copy()
    losses = _iterate(mem, ppo)
    seen = dict(count=mem.count, obs=mem.obs.cpu().numpy(), rew=mem.rew.cpu().numpy(), done=mem.done.cpu().numpy(),
                skip=mem.skip.cpu().numpy(), ended=mem.ended.cpu().numpy(), values=ppo.values.cpu().numpy(),
                ratio=ppo.first_ratio.cpu().numpy(), out=[t.cpu().numpy() for t in ppo.advantages.outputs],
                stats=[float(x) for x in ppo.advantages.stats], record=ppo.norm._record.cpu().numpy().view(np.uint64).copy(),
                carry=ppo.norm.carry.cpu().numpy(), folded=(ppo.norm.folded_obs, ppo.norm.folded_ret), empty=empty,
                scaled=ppo.norm._rew_ring.cpu().numpy(), losses={k: v for k, v in losses.items()})
    folder = tempfile.mkdtemp(prefix="uavx_ppo_norm_")
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


def _reference(seen):
    """norm_ref's record after the update's fold_returns, after its fold_obs, and the carry."""
    ring = dict(done=seen["done"], learners=N, skip=seen["skip"], ended=seen["ended"], first=0, count=seen["count"])
    rec, C = norm_ref.fold_returns(norm_ref.new_record(10), np.zeros((E, N)), seen["rew"], gamma=0.99, **ring)
    return rec, norm_ref.fold_obs(rec, seen["obs"], **ring), C


@HEADS
def test_the_first_minibatch_of_the_first_epoch_has_ratio_one(fused):
    seen, _, _ = _run(fused, "a")
    ratio = seen["ratio"]
    print("first minibatch: ratio min", ratio.min(), "max", ratio.max(), "rows != 1:", int((ratio != 1.0).sum()), "of", ratio.size)
    assert ratio.shape == (T * E * N // 4,) and np.all(ratio == np.float32(1.0))


@HEADS
def test_the_update_used_the_reference_advantages_of_the_scaled_rewards(fused):
    seen, _, _ = _run(fused, "a")
    assert seen["count"] == T and not seen["empty"].any()
    rec, _, _ = _reference(seen)
    scaled = norm_ref.scale_rewards(rec, seen["rew"])
    assert same(seen["scaled"], scaled)
    assert rec["n_ret"] > 0 and not np.array_equal(scaled, seen["rew"])      # the scale was defined at the first update
    kw = dict(rew=scaled, done=seen["done"], values=seen["values"], count=seen["count"], steps=T, gamma=0.99, lam=0.95,
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


@HEADS
def test_the_record_after_the_update_is_the_references(fused):
    seen, _, _ = _run(fused, "a")
    _, rec, C = _reference(seen)
    assert norm_ref.same_words(seen["record"], norm_ref.words(rec)) and same(seen["carry"], C)
    assert seen["folded"] == (T, T) and 0 < rec["n_obs"] == rec["n_ret"] < T * E * N


@HEADS
def test_two_learners_from_the_same_seeds_are_byte_equal(fused):
    (_, _, a), (_, _, b) = _run(fused, "a"), _run(fused, "b")
    assert _equal(a, b)
    assert all(bool(torch.isfinite(x.float()).all()) for x in a[:-3])


@HEADS
def test_a_saved_run_resumes_to_the_same_bytes(fused):
    from gym_uav_collision_avoidance_amd.checkpoint import load_run
    _, path, final = _run(fused, "a")
    env, mem, gen, ppo = _build(fused, torch_seed=99)                        # other initial weights: the file must bring them
    gen.manual_seed(1234)
    extra = load_run(path, env=env, memory=mem, agent=ppo, generator=gen)
    assert extra == {"t": T} and mem.count == T and ppo.updates == 1
    assert (ppo.norm.folded_obs, ppo.norm.folded_ret) == (T, T) and int(ppo.norm.stats.n_obs) > 0
    _iterate(mem, ppo)
    assert _equal(_state(mem, ppo), final)
    env.close()


def test_a_learner_without_normalisation_refuses_the_saved_state():
    from gym_uav_collision_avoidance_amd.checkpoint import load_run
    seen, path, _ = _run(False, "a")
    env, mem, gen, plain = _build(False, torch_seed=99, normalised=False)
    before = [p.detach().clone() for p in plain.params]
    with pytest.raises(ValueError, match="with normalisation, this one is built without"):
        load_run(path, env=env, memory=mem, agent=plain, generator=gen)
    assert all(torch.equal(a, b) for a, b in zip(before, plain.params)) and "norm" not in plain.state_dict()
    env2, mem2, gen2, normed = _build(False, torch_seed=98)
    with pytest.raises(ValueError, match="without normalisation, this one is built with"):
        normed.load_state_dict(plain.state_dict())
    env.close()
    env2.close()


@HEADS
def test_select_action_is_the_policy_on_normalised_observations(fused):
    env, mem, gen, ppo = _build(fused)
    _iterate(mem, ppo)
    x = (torch.randn((33, 10), generator=torch.Generator().manual_seed(2)) * 3).to(DEV)
    with torch.no_grad():
        want = ppo.policy.act(ppo.norm.obs(x), evaluate=True, generator=gen)
    got = ppo.select_action(x)
    assert torch.equal(got, want) and not torch.equal(got, ppo.policy.act(x, evaluate=True, generator=gen))
    rec = ppo.norm._record.cpu().numpy().view(np.uint64)
    assert same(ppo.norm.obs(x).cpu().numpy(),
                norm_ref.apply_obs(dict(n_obs=int(rec[0]), mean=rec[1:11].view(np.float64), M2=rec[17:27].view(np.float64),
                                        n_ret=0, mean_ret=0.0, M2_ret=0.0), x.cpu().numpy()))
    env.close()

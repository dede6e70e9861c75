"""PPO on the device ring (ppo.py) on the MI355X, 64 envs x 2 agents, T = 8: two learners built from the same
seeds are byte-equal after two rollouts and updates; the advantages an update used are gae_ref's on the ring it saw; the
probability ratio over the first minibatch of the first epoch is exactly 1; a learner saved after an update and loaded into a
fresh one continues to the same bytes.  No test asserts that a policy learns."""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import gae_ref
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

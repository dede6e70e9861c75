"""Generation-time only: drives the REFERENCE's learners (pytorch_sac_temp/sac.py, pytorch_td3_temp/td3.py,
pytorch_ddpg_temp/ddpg.py, imported by path as ref_loader.py does for the envs) through their real update_parameters on
the CPU and records what the learner tests compare against in tests/golden/learner_updates_{sac,td3,ddpg}.npz.  No test
imports the reference; nothing of it is copied here, and only data goes into the files.

    python tests/golden/make_learner_updates.py            # needs the reference checkout (UAVX_REFERENCE_ROOT)

Per learner and per case (K = 6 updates at B = 32 and at B = 17), from the recipe weights of tests/learner_ref.py:
    b{B}_state, _action, _reward, _next_state, _mask     the batches a scripted memory hands the reference [K, B, ...]
    b{B}_noise                                           the standard-normal draws fed to it [K, n, B, 2] (SAC's two
                                                         rsample calls, TD3's randn_like, none for DDPG)
    b{B}_scalars_ref                                     what update_parameters returned, in the loss ring's columns
                                                         (NaN where the reference returns nothing: all of TD3)
    b{B}_scalars_f64, _scalars_f32                       the restatement's own, in float64 and float32
    idx_{tensor}                                         256 fixed indices per tensor (all of a smaller one)
    meta                                                 JSON: kind "learner_updates", the learner, K, the row counts
    b{B}_f32_{tensor}, b{B}_f64_{tensor}                 the reference's float32 final parameters and the float64
                                                         restatement's at those indices
The reference's SAC reads target_entropy from uninitialised memory (sac.py:29); it is set to -2.0 here after
construction, the value FusedSAC and the restatement use."""
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import learner_ref as lr  # noqa: E402
from ref_loader import REF_ROOT  # noqa: E402
NOISES = {"sac": 2, "td3": 1, "ddpg": 0}


class ScriptedMemory:
    """memory.sample(batch_size) hands out the recorded batches in order, as the reference's ReplayMemory returns them."""

    def __init__(self, batches):
        self.batches, self.k = batches, 0

    def sample(self, batch_size):
        b = self.batches[self.k]
        assert b[0].shape[0] == batch_size
        self.k += 1
        return b


class FedNoise:
    """Stands in for torch.distributions.normal._standard_normal / torch.randn_like: returns the recorded draws."""

    def __init__(self, draws):
        self.draws, self.k = draws, 0

    def __call__(self, *args, **kw):
        d = self.draws[self.k]
        self.k += 1
        return torch.from_numpy(d)


def inputs(kind, rows):
    rs = np.random.RandomState(lr.SEEDS[kind] + rows)
    batches, noises = [], []
    for _ in range(lr.K):
        s = rs.uniform(-1, 1, (rows, 10)).astype(np.float32)
        a = rs.uniform(-1, 1, (rows, 2)).astype(np.float32)
        r = rs.normal(0, 1, rows).astype(np.float32)
        s2 = rs.uniform(-1, 1, (rows, 10)).astype(np.float32)
        m = (rs.uniform(0, 1, rows) > 0.1).astype(np.float32)
        batches.append((s, a, r, s2, m))
        noises.append(tuple(rs.normal(0, 1, (rows, 2)).astype(np.float32) for _ in range(NOISES[kind])))
    return batches, noises


def reference_run(kind, batches, noises):
    """The reference's own float32 run -> ({tensor name: tensor}, scalars [K, 5] with NaN where nothing is returned)."""
    sys.path.insert(0, REF_ROOT)
    rows = batches[0][0].shape[0]
    mem = ScriptedMemory(batches)
    out = np.full((lr.K, lr.COLUMNS), np.nan)
    fed = FedNoise([n for ns in noises for n in ns])
    if kind == "sac":
        agent = importlib.import_module("pytorch_sac_temp.sac").SAC(10, 2, cpu=True)
        agent.target_entropy = -2.0
        lr.load_recipe(agent, kind)
        normal = importlib.import_module("torch.distributions.normal")
        keep, normal._standard_normal = normal._standard_normal, fed
        try:
            for u in range(lr.K):
                out[u] = agent.update_parameters(mem, rows, u)
        finally:
            normal._standard_normal = keep
        nets = {k: getattr(agent, k) for k in ("policy", "critic", "critic_target")}
    elif kind == "td3":
        agent = importlib.import_module("pytorch_td3_temp.td3").TD3(10, 2)
        lr.load_recipe(agent, kind)
        keep, torch.randn_like = torch.randn_like, fed
        try:
            for u in range(lr.K):
                assert agent.update_parameters(mem, rows, u) is None
        finally:
            torch.randn_like = keep
        nets = {k: getattr(agent, k) for k in ("actor", "actor_target", "critic", "critic_target")}
    else:
        agent = importlib.import_module("pytorch_ddpg_temp.ddpg").DDPG(10, 2)
        lr.load_recipe(agent, kind)
        for u in range(lr.K):
            actor_loss, critic_loss = agent.update_parameters(mem, rows)
            out[u] = [critic_loss, 0.0, actor_loss, 0.0, 0.0]
        nets = {k: getattr(agent, k) for k in ("actor", "actor_target", "critic", "critic_target")}
    assert fed.k == len(fed.draws) and mem.k == lr.K
    tensors = {f"{k}.{n}": p.detach() for k, m in nets.items() for n, p in m.named_parameters()}
    if kind == "sac":
        tensors["log_alpha"] = agent.log_alpha.detach()
    return tensors, out


def main():
    torch.set_num_threads(1)
    for kind in lr.KINDS:
        idx = lr.sample_indices(kind)
        data = {f"idx_{n}": v.astype(np.int32) for n, v in idx.items()}
        # every fixture of tests/golden carries a `meta` entry with its kind (tests/golden_util.py lists them by it)
        data["meta"] = np.array(json.dumps(dict(kind="learner_updates", learner=kind, updates=lr.K, rows=list(lr.CASES),
                                                target_entropy=lr.TARGET_ENTROPY, seeds=lr.SEEDS[kind])))
        for rows in lr.CASES:
            batches, noises = inputs(kind, rows)
            p = f"b{rows}_"
            for j, k in enumerate(("state", "action", "reward", "next_state", "mask")):
                data[p + k] = np.stack([b[j] for b in batches])
            data[p + "noise"] = np.stack([np.stack(n) if n else np.zeros((0, rows, 2), np.float32) for n in noises])
            tensors, scalars = reference_run(kind, batches, noises)
            l64, s64 = lr.run(kind, batches, noises, torch.float64)
            _, s32 = lr.run(kind, batches, noises, torch.float32)
            data[p + "scalars_ref"], data[p + "scalars_f64"], data[p + "scalars_f32"] = scalars, s64, s32
            for n, v in lr.sampled(tensors, idx).items():
                data[p + "f32_" + n] = v.astype(np.float32)
            for n, v in lr.sampled(l64.tensors(), idx).items():
                data[p + "f64_" + n] = v
            print(kind, rows, "reference scalars\n", scalars, "\nfloat64 restatement\n", s64)
        path = os.path.join(HERE, f"learner_updates_{kind}.npz")
        np.savez_compressed(path, **data)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

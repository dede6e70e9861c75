"""The learners' gradient launches (FusedCriticLoss.backward, FusedActionGrad.q_dqda, FusedPolicyGrad.act + backward_from)
write the same bits as the commit that recorded tests/golden/grad_bits_parent.json: sha256 of the raw bytes of every output
(gradients, losses, q, dq/da, action, log_pi), with no tolerance.  The kernels are deterministic by design (fixed summation
orders, test_determinism_* of the three units' GPU tests), so a change that only moves code must leave every digest as it is.

Weights and inputs come from numpy.random.RandomState (the frozen legacy generator), never from torch's generators or
initialisers: the fixture does not depend on the torch version.

Rows: 1 (a lone row), 17 (a ragged second block), 145 (b16 = 160, kc = 64, S = 3 with a short last slice: the smallest count
at which the split-K path and its slice clamp run).  Hidden sizes: each learner's default and an odd one inside the accepted
range, where the padding lanes of every shared piece run.

Recording, at the commit whose bits are to be kept (this file uses only classes that commit has):

    python tests/test_gpu_grad_bits.py --record tests/golden/grad_bits_parent.json --commit <id>
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import policy_grad_ref as ref                                                      # noqa: E402
from grad_ref import critic                                                        # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "grad_bits_parent.json")
KINDS = ["sac", "td3", "ddpg"]
ROWS = (1, 17, 145)
SHAPES = {"sac": ((256, 256), (243, 70)), "td3": ((256, 256), (243, 70)), "ddpg": ((400, 300), (387, 33))}
CELLS = [(k, h1, h2) for k in KINDS for h1, h2 in SHAPES[k]]


def _fill(module, rs):
    """Every parameter from rs: weights N(0, 1 / fan_in), biases 0.1 N(0, 1)."""
    with torch.no_grad():
        for p in module.parameters():
            v = rs.standard_normal(tuple(p.shape))
            v *= 0.1 if p.dim() == 1 else 1.0 / np.sqrt(p.shape[1])
            p.copy_(torch.from_numpy(v.astype(np.float32)))
    return module


def _dev(rs_array, dev):
    return torch.from_numpy(np.ascontiguousarray(rs_array, dtype=np.float32)).to(dev)


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def digests(kind, h1, h2, dev=None):
    """{rows: {output name: sha256}} of one learner at one hidden shape."""
    from gym_uav_collision_avoidance_amd.fused_critic import FusedActionGrad, FusedCriticLoss
    from gym_uav_collision_avoidance_amd.fused_policy_grad import FusedPolicyGrad
    dev = dev or torch.device("cuda", 0)
    rs = np.random.RandomState(1000 * KINDS.index(kind) + h1 + h2)
    crit = _fill(critic(kind, 0, hidden1=h1, hidden2=h2), rs).to(dev)
    pol = _fill(ref.actor_with(kind, 0, hidden1=h1, hidden2=h2), rs).to(dev)
    closs, ag = FusedCriticLoss(crit), FusedActionGrad(crit)
    pg = FusedPolicyGrad(pol, ag)
    out = {}
    for rows in ROWS:
        s, a = _dev(rs.standard_normal((rows, 10)), dev), _dev(rs.uniform(-1.0, 1.0, (rows, 2)), dev)
        y, eps = _dev(rs.standard_normal(rows), dev), _dev(rs.standard_normal((rows, 2)), dev)
        d = {}
        losses = closs.backward(s, a, y)
        for i, l in enumerate(losses if isinstance(losses, tuple) else (losses,)):
            d[f"critic_loss{i}"] = _sha(l)
        for i, p in enumerate(crit.parameters()):
            d[f"critic_grad{i}"] = _sha(p.grad)
        action, log_pi = pg.act(s, noise=eps if kind == "sac" else None)
        d["action"] = _sha(action)
        q, j = ag.q_dqda(s, action)
        d["q"], d["dqda"] = _sha(q), _sha(j)
        res = pg.backward_from(s, q, j, alpha=0.2 if kind == "sac" else None)
        d["actor_loss"] = _sha(res[0] if kind == "sac" else res)
        if kind == "sac":
            d["log_pi"], d["log_pi_mean"] = _sha(log_pi), _sha(pg.log_pi_mean)
        for i, p in enumerate(pol.parameters()):
            d[f"actor_grad{i}"] = _sha(p.grad)
        torch.cuda.synchronize()
        out[str(rows)] = d
    pg.close()
    ag.close()
    closs.close()
    return out


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["cells"]


@pytest.mark.parametrize("kind,h1,h2", CELLS)
def test_every_output_bit_equals_the_recorded_commit(kind, h1, h2):
    want = _golden()[f"{kind}/{h1}x{h2}"]
    got = digests(kind, h1, h2)
    assert sorted(got) == sorted(want) == sorted(str(r) for r in ROWS)
    for rows in got:
        assert sorted(got[rows]) == sorted(want[rows]), (kind, h1, h2, rows)
        # losses, q, dq/da, action (and log_pi), every gradient
        assert len(got[rows]) == {"sac": 28, "td3": 24, "ddpg": 17}[kind]
        bad = [n for n in got[rows] if got[rows][n] != want[rows][n]]
        assert not bad, f"{kind} {h1}x{h2}, {rows} rows: other bits than the recorded commit in {bad}"


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, metavar="JSON")
    ap.add_argument("--commit", required=True, help="the commit the library under this file was built from")
    args = ap.parse_args()
    cells = {f"{k}/{h1}x{h2}": digests(k, h1, h2) for k, h1, h2 in CELLS}
    os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
    with open(args.record, "w") as f:
        json.dump({"commit": args.commit, "cells": cells}, f, indent=1, sort_keys=True)
        f.write("\n")
    count = sum(len(d) for c in cells.values() for d in c.values())
    print(f"recorded {count} digests of {len(cells)} cells to {args.record}")

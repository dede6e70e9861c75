"""FusedCriticLoss.backward(weight=, q_out=) writes the same bits as the commit that recorded
tests/golden/wgrad_bits_parent.json: sha256 of the raw bytes of every gradient, every loss and q, with no tolerance.  The
weighted and the unweighted call are two instantiations of one row kernel, so "a weight of 1 equals the unweighted call"
(test_gpu_wgrad.py) compares the source with itself; this fixture is the anchor outside the tree: it was recorded while the
weighted call was a library of its own.  test_gpu_grad_bits.py is the same anchor for the unweighted call.

Weights and inputs come from numpy.random.RandomState (the frozen legacy generator), never from torch's generators or
initialisers: the fixture does not depend on the torch version.

Cells, rows and hidden sizes are test_gpu_grad_bits.py's (145 rows: the smallest count at which the split-K path runs, with a
short last slice); both losses; three calls each:
    none_q    weight=None, q_out=q
    w_q       weight=w [B] uniform in [0, 2), the first and the last row exactly 0 (rows > 1), q_out=q
    col_noq   weight= the middle [B, 1] column of a [B, 3] tensor (row stride 3), q_out=None

Recording, at the commit whose bits are to be kept (this file uses only classes that commit has):

    python tests/test_gpu_wgrad_bits.py --record tests/golden/wgrad_bits_parent.json --commit <id>
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from grad_ref import critic                                                        # noqa: E402
from test_gpu_grad_bits import CELLS, KINDS, ROWS, _dev, _fill, _sha               # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_bits_parent.json")
LOSSES = ("mse", "l1")
CALLS = ("none_q", "w_q", "col_noq")


def digests(kind, h1, h2, dev=None):
    """{"rows/loss/call": {output name: sha256}} of one critic at one hidden shape."""
    from gym_uav_collision_avoidance_amd.fused_critic import FusedCriticLoss
    dev = dev or torch.device("cuda", 0)
    rs = np.random.RandomState(7000 + 1000 * KINDS.index(kind) + h1 + h2)
    crit = _fill(critic(kind, 0, hidden1=h1, hidden2=h2), rs).to(dev)
    out = {}
    for loss in LOSSES:
        closs = FusedCriticLoss(crit, loss=loss)
        T = closs.critic.towers
        for rows in ROWS:
            s, a = _dev(rs.standard_normal((rows, 10)), dev), _dev(rs.uniform(-1.0, 1.0, (rows, 2)), dev)
            y = _dev(rs.standard_normal(rows), dev)
            w = rs.uniform(0.0, 2.0, rows)
            if rows > 1:
                w[0] = w[-1] = 0.0
            wide = rs.uniform(0.0, 2.0, (rows, 3))
            w, col = _dev(w, dev), _dev(wide, dev)[:, 1:2]
            assert rows == 1 or (col.stride(0) == 3 and float(w[0]) == 0.0 == float(w[-1]))
            for call in CALLS:
                q = None if call == "col_noq" else torch.full((T, rows), float("nan"), device=dev)
                weight = {"none_q": None, "w_q": w, "col_noq": col}[call]
                losses = closs.backward(s, a, y, weight=weight, q_out=q)
                d = {f"loss{i}": _sha(l) for i, l in enumerate(losses if isinstance(losses, tuple) else (losses,))}
                for i, p in enumerate(crit.parameters()):
                    d[f"grad{i}"] = _sha(p.grad)
                if q is not None:
                    d["q"] = _sha(q)
                torch.cuda.synchronize()
                out[f"{rows}/{loss}/{call}"] = d
        closs.close()
    return out


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["cells"]


def test_the_fixture_holds_these_cells_and_no_others():
    assert sorted(_golden()) == sorted(f"{k}/{h1}x{h2}" for k, h1, h2 in CELLS)


@pytest.mark.parametrize("kind,h1,h2", CELLS)
def test_every_weighted_output_bit_equals_the_recorded_commit(kind, h1, h2):
    want = _golden()[f"{kind}/{h1}x{h2}"]
    got = digests(kind, h1, h2)
    assert sorted(got) == sorted(want) == sorted(f"{r}/{l}/{c}" for r in ROWS for l in LOSSES for c in CALLS)
    towers = 1 if kind == "ddpg" else 2
    for name in got:
        assert sorted(got[name]) == sorted(want[name]), (kind, h1, h2, name)
        # every tower's loss and six gradients, and q where the call asked for it
        assert len(got[name]) == 7 * towers + (0 if name.endswith("col_noq") else 1)
        bad = [n for n in got[name] if got[name][n] != want[name][n]]
        assert not bad, f"{kind} {h1}x{h2}, {name}: other bits than the recorded commit in {bad}"


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, metavar="JSON")
    ap.add_argument("--commit", required=True, help="the commit the libraries under this file were built from")
    args = ap.parse_args()
    cells = {f"{k}/{h1}x{h2}": digests(k, h1, h2) for k, h1, h2 in CELLS}
    os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
    with open(args.record, "w") as f:
        json.dump({"commit": args.commit, "cells": cells}, f, indent=1, sort_keys=True)
        f.write("\n")
    count = sum(len(d) for c in cells.values() for d in c.values())
    print(f"recorded {count} digests of {len(cells)} cells to {args.record}")

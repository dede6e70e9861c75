"""Generation-time only: runs the REFERENCE's Ornstein-Uhlenbeck class (pytorch_ddpg_temp/ou.py, imported by path from the
checkout ref_loader.py names) as ddpg.py:31 constructs it and records what the exploration tests compare against in
tests/golden/ou_reference.npz.  No test imports the reference; nothing of it is copied here, and only data goes into the file.

    python tests/golden/make_explore_golden.py            # needs the reference checkout (UAVX_REFERENCE_ROOT)

Per case i of tests/explore_ref.py's OU_CASES (np.random.seed(s), std_deviation sigma), K = 512 calls:
    case{i}_normals    the K standard normals np.random.normal(size=(1,)) hands the class, float64 [K]
    case{i}_x          what the K calls returned, float64 [K]
    meta               JSON: kind "ou_reference", the cases, K, theta, dt, mean
The generator also runs 4096 calls per case and requires the restatement (explore_ref.ou_run) to equal the class bit for
bit on all of them, so the tests' comparison with the fixture is an equality."""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import explore_ref as er  # noqa: E402
from ref_loader import REF_ROOT  # noqa: E402

LONG = 4096


def reference_class():
    spec = importlib.util.spec_from_file_location("uavx_reference_ou", os.path.join(REF_ROOT, "pytorch_ddpg_temp", "ou.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.OUActionNoise


def run_case(cls, seed, sigma, steps):
    np.random.seed(seed)
    z = np.array([np.random.normal(size=(1,))[0] for _ in range(steps)], dtype=np.float64)
    np.random.seed(seed)
    proc = cls(mean=np.zeros(1), std_deviation=float(sigma) * np.ones(1))           # ddpg.py:31
    x = np.array([proc()[0] for _ in range(steps)], dtype=np.float64)
    return z, x


def main():
    cls = reference_class()
    out = {}
    for i, (seed, sigma) in enumerate(er.OU_CASES):
        z, x = run_case(cls, seed, sigma, LONG)
        mine = er.ou_run(z, sigma)
        assert np.array_equal(mine, x), f"case {i}: the restatement leaves the reference at call {int(np.argmax(mine != x))}"
        out[f"case{i}_normals"], out[f"case{i}_x"] = z[:er.OU_STEPS], x[:er.OU_STEPS]
    out["meta"] = np.array(json.dumps({"kind": "ou_reference", "cases": [list(c) for c in er.OU_CASES], "steps": er.OU_STEPS,
                                       "theta": er.OU_THETA, "dt": er.OU_DT, "mean": er.OU_MEAN, "checked_steps": LONG}))
    path = os.path.join(HERE, "ou_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

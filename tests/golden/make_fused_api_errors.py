"""Generation-time only: runs the case list of tests/test_gpu_fused_api_errors.py (its CASES, not a second list) on the
GPU and writes what each case raised, {case id: [exception class name, message]}, to fused_api_errors_parent.json.  The
file in the repository was recorded once with the package as it stood at commit 1ba5a5c, before the bindings' argument
checks moved into _fused_common.py; the test holds every later tree to it.

    PYTHONPATH=<a checkout of 1ba5a5c, libraries built> python tests/golden/make_fused_api_errors.py --record [--out FILE]

The package is imported from PYTHONPATH when it is there and from this tree otherwise; the path used is printed."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/: the case list
sys.path.append(os.path.dirname(os.path.dirname(HERE)))         # this tree's package, behind PYTHONPATH


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", help="run the cases and write the file (the default prints only)")
    ap.add_argument("--out", default=os.path.join(HERE, "fused_api_errors_parent.json"))
    a = ap.parse_args()
    import gym_uav_collision_avoidance_amd as pkg
    import test_gpu_fused_api_errors as t
    print("package:", os.path.dirname(os.path.abspath(pkg.__file__)), flush=True)
    rec = {name: t.outcome(fn) for name, fn in sorted(t.CASES.items())}
    silent = [name for name, (cls, _) in rec.items() if not cls]
    print(f"{len(rec)} cases, {len(silent)} raised nothing: {silent}", flush=True)
    if a.record:
        if silent:
            raise SystemExit("not recorded: every case must be a rejection")
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", a.out)
    else:
        print(json.dumps(rec, indent=0, sort_keys=True))


if __name__ == "__main__":
    main()

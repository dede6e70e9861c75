"""Host-side checks of the exploration launch (include/uavx_explore.h, gym_uav_collision_avoidance_amd/exploration.py): the
header declares what _actor_lib binds, the library cross-compiles with the new unit under the source hash and exports it,
the kernels use no scratch, every documented rejection happens before a device is touched, the fixture holds the
reference's Ornstein-Uhlenbeck runs and the restatement (tests/explore_ref.py) equals them bit for bit, and the restated
normals have the moments and the bound of the Box-Muller map they state."""
import ctypes
import importlib.util
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import explore_ref as er
from reset_layouts import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _alib():
    from gym_uav_collision_avoidance_amd import _actor_lib
    _actor_lib.build()
    return _actor_lib


def test_explore_exports_every_declared_symbol():
    a = _alib()
    hdr = open(a.EXPLORE_HEADER).read()
    declared = set(re.findall(r"\b(uavx_explore[a-z_0-9]*)\s*\(", hdr))
    assert declared == set(a.EXPLORE_SYMBOLS), declared ^ set(a.EXPLORE_SYMBOLS)
    assert set(a.EXPLORE_SYMBOLS).isdisjoint(a.SYMBOLS + a.CRITIC_SYMBOLS + a.GRAD_SYMBOLS + a.OPTIM_SYMBOLS + a.REPLAY_SYMBOLS
                                             + a.ACTION_GRAD_SYMBOLS + a.POLICY_GRAD_SYMBOLS + a.LEARNER_SYMBOLS)
    lib = a.load()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.uavx_explore_version() == a.EXPLORE_ABI_VERSION == 1
    assert "#define UAVX_EXPLORE_VERSION 1" in hdr
    assert f"#define UAVX_EXPLORE_MAX_ROWS {a.EXPLORE_MAX_ROWS}" in hdr and a.EXPLORE_MAX_ROWS == 2 ** 24
    assert f"#define UAVX_EXPLORE_STATE_BYTES {a.EXPLORE_STATE_BYTES}" in hdr


def test_args_structure_has_the_headers_fields_in_order():
    a = _alib()
    hdr = open(a.EXPLORE_HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", hdr.split("typedef struct uavx_explore_args {", 1)[1].split("} uavx_explore_args;", 1)[0],
                  flags=re.S)
    names = []
    for decl in body.split(";"):
        parts = [re.sub(r"[\s*]", "", p.split()[-1] if p.split() else "") for p in decl.split(",")]
        names += [p for p in parts if p]
    assert names == [f[0] for f in a.ExploreArgs._fields_]
    assert ctypes.sizeof(a.ExploreArgs) == 176 and a.ExploreArgs.ou_sigma.offset == 136


def test_explore_library_cross_compiles_and_hash_covers_header():
    a = _alib()
    assert a.EXPLORE_HEADER in a._sources()
    assert any(f.endswith("uavx_explore.hip") for f in a._sources())
    assert f"UAVX_ACTOR_SRC_HASH={a.source_hash()}".encode() in open(a.LIB_PATH, "rb").read()
    mk = open(os.path.join(a.CSRC, "Makefile")).read()
    assert "uavx_explore.hip" in mk and "uavx_explore.h" in mk and "-ffp-contract=off" in mk
    nm = subprocess.run(["nm", "-D", "--defined-only", a.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert set(a.EXPLORE_SYMBOLS) <= exported
    assert {s for s in exported if s.startswith("uavx_explore")} == set(a.EXPLORE_SYMBOLS)


def test_explore_kernels_use_no_scratch_and_no_lds():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.kernel_table(_alib().LIB_PATH)
    mine = sorted((r for r in rows if r["name"].startswith("uavx_explore_k::")), key=lambda r: r["name"])
    assert [r["name"] for r in mine] == [f"uavx_explore_k::act<{k}>" for k in (0, 1, 2)]
    rec = json.load(open(os.path.join(ROOT, "profiles", "r16_explore_kernel_resources.json")))
    assert [x["name"] for x in rec] == [r["name"] for r in mine]
    for r, x in zip(mine, rec):
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0
        assert r["max_flat_workgroup_size"] == 256
        for f in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                  "max_flat_workgroup_size"):
            assert x[f] == r[f], (r["name"], f, x[f], r[f])
    # the other units keep their kernels
    assert sum(x["name"].startswith("uavx_learner_k::") for x in rows) == 1
    assert sum(x["name"].startswith("uavx_optim_k::") for x in rows) == 3


def test_bad_arguments_rejected_before_any_device_call():
    a = _alib()
    lib = a.load()
    from gym_uav_collision_avoidance_amd.exploration import launch
    P = 4096                     # never dereferenced: every call that gets it fails its argument check first
    nan, inf = float("nan"), float("inf")

    def act(**kw):
        f = dict(kind=a.TD3, rows=64, raw=P, raw_stride=2, out=P, out_stride=2, state=P, noise_std=0.1, ou_sigma=0.2,
                 ou_theta=0.15, ou_dt=1e-2)
        f.update(kw)
        return launch(lib, None, **f)

    bad = a.ERR_INVALID_ARG
    assert lib.uavx_explore_act(None, None) == bad
    assert act(rows=0) == bad and act(rows=-1) == bad and act(rows=a.EXPLORE_MAX_ROWS + 1) == bad
    for name in ("raw", "out", "state"):
        assert act(**{name: None}) == bad, name
    assert act(state=P + 8) == bad
    assert act(kind=a.SAC, raw_stride=4, raw=P + 8) == bad and act(kind=a.SAC, raw_stride=6) == bad
    assert act(kind=a.SAC, raw_stride=2) == bad
    assert act(raw=P + 4) == bad and act(raw_stride=3) == bad and act(raw_stride=0) == bad
    assert act(kind=a.DDPG, raw=P + 4) == bad
    assert act(out=P + 4) == bad and act(out_stride=3) == bad and act(out_stride=0) == bad
    assert act(normals=P + 8) == bad and act(normals_out=P + 8) == bad
    assert act(kind=3) == bad and act(kind=-1) == bad
    assert act(random_prob=-0.1) == bad and act(random_prob=1.5) == bad and act(random_prob=nan) == bad
    for name in ("noise_std", "ou_sigma", "ou_dt"):
        for v in (-1e-3, nan, inf):
            assert act(**{name: v}) == bad, (name, v)
    for name in ("ou_theta", "ou_mean", "ou_x_initial"):
        for v in (nan, inf, -inf):
            assert act(**{name: v}) == bad, (name, v)
    fl = dict(reset_flags=P, reset_stride=1, reset_mask=1, rows_per_env=4)
    assert act(**dict(fl, rows_per_env=0)) == bad and act(**dict(fl, rows_per_env=-4)) == bad
    assert act(**dict(fl, rows_per_env=3)) == bad                       # 64 rows are no multiple of 3
    assert act(**dict(fl, reset_mask=0)) == bad and act(**dict(fl, reset_mask=256)) == bad
    assert act(**dict(fl, reset_mask=-1)) == bad and act(**dict(fl, reset_stride=0)) == bad
    assert act(row_offset=-1) == bad and act(warmup_steps=-1) == bad


def test_python_wrapper_refuses_bad_arguments_before_the_device():
    from gym_uav_collision_avoidance_amd.exploration import Exploration
    with pytest.raises(TypeError, match="FusedActor"):
        Exploration(object(), 4)


def test_fixture_holds_only_the_documented_arrays():
    meta, fx = er.load_fixture(GOLDEN)
    assert set(fx) == {f"case{i}_{n}" for i in range(3) for n in ("normals", "x")}
    assert meta["kind"] == "ou_reference" and meta["steps"] == er.OU_STEPS == 512
    assert [tuple(c) for c in meta["cases"]] == list(er.OU_CASES) == [(0, 0.2), (7, 0.2), (3, 1.5)]
    assert (meta["theta"], meta["dt"], meta["mean"]) == (er.OU_THETA, er.OU_DT, er.OU_MEAN) == (0.15, 1e-2, 0.0)
    for v in fx.values():
        assert v.dtype == np.float64 and v.shape == (512,) and np.isfinite(v).all()
    assert os.path.getsize(os.path.join(GOLDEN, "ou_reference.npz")) < 64 * 1024
    # the recorded normals are numpy's for the case's seed: the file is the reference's run, not the restatement's
    for i, (seed, _) in enumerate(er.OU_CASES):
        assert np.array_equal(np.random.RandomState(seed).normal(size=512), fx[f"case{i}_normals"])


@pytest.mark.parametrize("case", range(3))
def test_restated_ou_is_bit_equal_to_the_reference(case):
    _, fx = er.load_fixture(GOLDEN)
    sigma = er.OU_CASES[case][1]
    x = er.ou_run(fx[f"case{case}_normals"], sigma)
    assert np.array_equal(x, fx[f"case{case}_x"])
    assert np.abs(x).max() > 0.05 * sigma            # the process moved
    # and act()'s DDPG branch is the same recurrence, one call at a time, on a row that never acts at random
    xs, n = np.zeros(1), np.zeros(1, dtype=np.uint32)
    raw = np.zeros((1, 2), dtype=np.float32)
    for k in range(32):
        _, xs, n, rnd, _ = er.act(er.DDPG, raw, xs, n, seed=1, sigma=sigma, fed=np.array([[fx[f"case{case}_normals"][k], 0.0]]))
        assert not rnd[0] and xs[0] == fx[f"case{case}_x"][k]
    assert n[0] == 32


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    def run(c, k):
        return [int(w[0]) for w in philox4x32_10(*[np.array([v]) for v in c], *k)]
    f = 0xFFFFFFFF
    assert run((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert run((f, f, f, f), (f, f)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert run((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_words_are_keyed_by_global_row_call_and_stream():
    w = er.words(0x0123456789ABCDEF, np.array([5, 2 ** 40 + 3], dtype=np.uint64), np.array([7, 9]), 1)
    for j, (g, n) in enumerate(((5, 7), (2 ** 40 + 3, 9))):
        want = philox4x32_10(np.array([g & 0xFFFFFFFF]), np.array([g >> 32]), np.array([n]), np.array([1]),
                             0x89ABCDEF, 0x01234567)
        assert [int(x[j]) for x in w] == [int(x[0]) for x in want]


def test_restated_normals_have_the_moments_and_the_bound():
    n = 1_000_000
    w = er.words(11, np.arange(n // 2, dtype=np.uint64), 0, 0)
    z = np.concatenate(er.normals(w[0], w[1]))
    assert z.size == n and np.isfinite(z).all()
    mean, var, top = float(z.mean()), float(z.var()), float(np.abs(z).max())
    print("normals: mean", mean, "var", var, "max |n|", top)
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert top <= er.MAX_NORMAL == 6.67
    assert math.sqrt(-2 * math.log(2.0 ** -32)) <= er.MAX_NORMAL          # the bound from u1 >= 2^-32
    # the extreme words: u1 = 2^-32 gives the largest radius, u1 = 1 gives zero
    lo, hi = er.normals(np.array([0], dtype=np.uint32), np.array([0], dtype=np.uint32))
    assert lo[0] == math.sqrt(-2 * math.log(2.0 ** -32)) and hi[0] == 0.0
    one = er.normals(np.array([0xFFFFFFFF], dtype=np.uint32), np.array([123], dtype=np.uint32))
    assert one[0][0] == 0.0 and one[1][0] == 0.0
    u = er.uniform_action(np.array([0, 2 ** 31, 0xFFFFFFFF], dtype=np.uint32))
    assert u.dtype == np.float32 and list(u) == [-1.0, 0.0, 1.0]


def test_decision_order_of_the_restatement():
    g = np.arange(4096, dtype=np.uint64)
    n = np.full(4096, 5, dtype=np.uint32)
    assert er.decide(3, g, n, 6, 0.0).all() and not er.decide(3, g, n, 5, 0.0).any()
    assert er.decide(3, g, n, 0, 1.0).all()                              # ub < 1 always
    half = er.decide(3, g, n, 0, 0.5)
    assert abs(int(half.sum()) - 2048) <= 5 * math.sqrt(4096 * 0.25)
    assert np.array_equal(half, er.bernoulli_u(er.words(3, g, n, 1)[0]) < 0.5)

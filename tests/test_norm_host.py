"""Host-side checks of the running statistics (libuavx_norm.so, include/uavx_norm.h): the numpy restatement the
GPU tests trust (norm_ref.py) equals a second, per-column writing of the header's prose bit for bit on every crafted layout,
in both flag layouts, for one fold and for three successive folds with a carried C; what the folds leave are the statistics
of the concatenated samples within the bound of a float64 sum; without cuts the carry is the discounted return; a restatement
that ignored `ended` or counted parked rows would miss by orders of magnitude; the sample rule is PPO's weight; the library
builds for gfx950 without a GPU, carries its source hash, exports exactly what its header declares and refuses every bad
argument before touching a device; the other libraries keep their hashes; the Python layers refuse bad arguments on the host
and a PPO without the switches is the PPO it was."""
import ctypes
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

import gae_layouts
import norm_layouts
import norm_ref
from gae_ref import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "gym_uav_collision_avoidance_amd"


def _xlib():
    from gym_uav_collision_avoidance_amd import _norm_lib
    _norm_lib.build()
    return _norm_lib


# ---- the restatement -------------------------------------------------------------------------------------------------------

def _fold_both(case, windows):
    """The record and carry after folding `windows` with either writing; asserts they are bit-equal and returns the first."""
    ra = norm_layouts.ring_args(case)
    F = case["F"]
    rec, rec2 = norm_ref.new_record(F), norm_ref.new_record(F)
    C = C2 = np.zeros((case["E"], case["N"]))
    for first, count in windows:
        kw = dict(first=first, count=count, **ra)
        rec, rec2 = norm_ref.fold_obs(rec, case["obs"], **kw), norm_ref.fold_obs_loop(rec2, case["obs"], **kw)
        rec, C = norm_ref.fold_returns(rec, C, case["rew"], gamma=case["gamma"], **kw)
        rec2, C2 = norm_ref.fold_returns_loop(rec2, C2, case["rew"], gamma=case["gamma"], **kw)
        assert norm_ref.same_words(norm_ref.words(rec), norm_ref.words(rec2)), (first, count)
        assert same(C, C2), (first, count)
    x = case["obs"][:2]
    assert same(norm_ref.apply_obs(rec, x, 1e-8, 10.0), norm_ref.apply_obs_loop(rec2, x, 1e-8, 10.0))
    assert same(norm_ref.scale_rewards(rec, case["rew"], 1e-8, 2.0), norm_ref.scale_rewards_loop(rec2, case["rew"], 1e-8, 2.0))
    return rec, C


@pytest.mark.parametrize("folds", ["one", "three"])
@pytest.mark.parametrize("flags", ["rows", "packed"])
@pytest.mark.parametrize("name", sorted(norm_layouts.LAYOUTS))
def test_restatement_equals_the_loop_bit_for_bit(name, flags, folds):
    case = norm_layouts.make(name)
    case = norm_layouts.packed(case) if flags == "packed" else case
    windows = [(case["first"], case["count"])] if folds == "one" else norm_layouts.thirds(case)
    rec, C = _fold_both(case, windows)
    masks = [norm_ref.sample_mask(case["done"], k, case["learners"], case["skip"], case["ended"])
             for k in range(case["first"], case["count"])]
    assert rec["n_obs"] == rec["n_ret"] == sum(int(m.sum()) for m in masks)
    assert not C[:, case["learners"]:].any()                                  # columns that do not learn keep their +0


@pytest.mark.parametrize("flags", ["rows", "packed"])
@pytest.mark.parametrize("case", ["row_groups_9_wrapped", "row_groups_17_from0", "60x5_l3", "F7"])
def test_restatement_equals_the_loop_at_the_gpu_shapes(case, flags):
    c = {"row_groups_9_wrapped": lambda: norm_layouts.row_groups(9, True),
         "row_groups_17_from0": lambda: norm_layouts.row_groups(17, False),
         "60x5_l3": lambda: norm_layouts.big(60, 5, 6, learners=3, seed=73),
         "F7": lambda: norm_layouts.big(70, 4, 5, learners=3, F=7)}[case]()
    c = norm_layouts.packed(c) if flags == "packed" else c
    rec, _ = _fold_both(c, norm_layouts.thirds(c))
    assert rec["n_obs"] > 100


def test_a_batch_without_a_sample_leaves_the_record_alone():
    c = norm_layouts.make("count_9")
    ra = norm_layouts.ring_args(c)
    rec = norm_ref.fold_obs(norm_ref.new_record(10), c["obs"], first=c["first"], count=c["count"], **ra)
    rec, C = norm_ref.fold_returns(rec, np.zeros((3, 2)), c["rew"], first=c["first"], count=c["count"], gamma=0.99, **ra)
    empty = norm_layouts.make("all_skip")
    ra = norm_layouts.ring_args(empty)
    for fold_obs, fold_ret in ((norm_ref.fold_obs, norm_ref.fold_returns), (norm_ref.fold_obs_loop, norm_ref.fold_returns_loop)):
        after = fold_obs(rec, empty["obs"], first=empty["first"], count=empty["count"], **ra)
        after, C2 = fold_ret(after, C, empty["rew"], first=empty["first"], count=empty["count"], gamma=0.99, **ra)
        assert np.array_equal(norm_ref.words(after), norm_ref.words(rec)) and not C2.any()      # every carry was cut
    fresh = norm_ref.new_record(10)
    mean, var, var_ret = norm_ref.variances(fresh)
    assert not mean.any() and (var == 1).all() and var_ret == 1.0             # n = 0 reads as mean 0, variance 1


def _samples(case, windows):
    """(obs samples [n, F], return samples [n]) of the folds, gathered by numpy indexing."""
    ra = norm_layouts.ring_args(case)
    L = case["T"] + 1
    xs, rs = [], []
    C = np.zeros((case["E"], case["N"]))
    for first, count in windows:
        rows, masks, C = norm_ref.returns(C, case["rew"], first=first, count=count, gamma=case["gamma"], **ra)
        for k, R, m in zip(range(first, count), rows, masks):
            xs.append(case["obs"][k % L].reshape(-1, case["F"])[m].astype(np.float64))
            rs.append(R[m])
    return np.concatenate(xs), np.concatenate(rs)


def _six_windows(case):
    first, count = case["first"], case["count"]
    cuts = [first + (count - first) * j // 6 for j in range(7)]
    return list(zip(cuts[:-1], cuts[1:]))


def _miss(rec, xs, rs):
    """The largest |got − numpy| in units of the bound n · 2^-52 (relative), over every mean and variance."""
    n = xs.shape[0]
    bound = n * 2.0 ** -52
    mean, var, var_ret = norm_ref.variances(rec)
    worst = 0.0
    for f in range(xs.shape[1]):
        a = xs[:, f]
        worst = max(worst, abs(mean[f] - a.mean()) / (bound * max(abs(a.mean()), np.abs(a).mean())),
                    abs(var[f] - np.var(a)) / (bound * np.var(a)))
    worst = max(worst, abs(rec["mean_ret"] - rs.mean()) / (bound * max(abs(rs.mean()), np.abs(rs).mean())),
                abs(var_ret - np.var(rs)) / (bound * np.var(rs)))
    return worst


@pytest.mark.parametrize("flags", ["rows", "packed"])
def test_folds_are_the_statistics_of_the_concatenated_samples(flags):
    """Six folds over 300 x 4, T = 18: mean and M2 / n against np.mean and np.var over all samples, within n · 2^-52
    relative -- the bound of test_documented_summation_order_against_numpy_two_pass_std -- the feature offset by 1e4 included."""
    case = norm_layouts.big(300, 4, 18, learners=3, seed=75)
    case = norm_layouts.packed(case) if flags == "packed" else case
    windows = _six_windows(case)
    ra = norm_layouts.ring_args(case)
    rec, C = norm_ref.new_record(case["F"]), np.zeros((300, 4))
    for first, count in windows:
        rec = norm_ref.fold_obs(rec, case["obs"], first=first, count=count, **ra)
        rec, C = norm_ref.fold_returns(rec, C, case["rew"], first=first, count=count, gamma=case["gamma"], **ra)
    xs, rs = _samples(case, windows)
    assert rec["n_obs"] == rec["n_ret"] == xs.shape[0] == rs.size > 8000
    assert abs(xs[:, norm_layouts.OFFSET_FEATURE].mean()) > 9e3
    worst = _miss(rec, xs, rs)
    print(f"n = {xs.shape[0]}, worst |got - numpy| / (n * 2^-52 relative) = {worst:.4f}")
    assert worst <= 1.0


def test_without_cuts_the_carry_is_the_discounted_return():
    c = norm_layouts.with_obs(gae_layouts._clean(4, 2, T=12, count=30, seed=82, gamma=0.97))
    L, g, first, count = 13, 0.97, c["first"], c["count"]
    rec, C = norm_ref.fold_returns(norm_ref.new_record(10), np.zeros((4, 2)), c["rew"], first=first, count=count, gamma=g,
                                   **norm_layouts.ring_args(c))
    assert rec["n_ret"] == 12 * 8
    terms = [g ** (count - 1 - j) * c["rew"][j % L].astype(np.float64) for j in range(first, count)]
    direct, scale = sum(terms), sum(np.abs(t) for t in terms)
    # per term one rounding of the product and one of the sum, each at most 2^-53 of a quantity bounded by `scale`
    assert np.all(np.abs(C - direct) <= 2 * 12 * 2.0 ** -53 * scale)
    # in two folds the carry passes the boundary: the same bits as in one
    rec2, C2 = norm_ref.new_record(10), np.zeros((4, 2))
    for a, b in ((first, first + 5), (first + 5, count)):
        rec2, C2 = norm_ref.fold_returns(rec2, C2, c["rew"], first=a, count=b, gamma=g, **norm_layouts.ring_args(c))
    assert same(C, C2) and rec2["n_ret"] == rec["n_ret"]


def test_the_statistics_see_a_wrong_sample_rule_or_recurrence():
    """The comparison with numpy has teeth: on ppo_ring a restatement that ignored `ended` (the carry runs through episode
    ends, and rows after an episode's end count as parked), or one that counted parked rows, misses by orders of magnitude."""
    case = norm_layouts.ppo_ring()
    windows = [(case["first"], case["count"])]
    ra = norm_layouts.ring_args(case)
    kw = dict(first=case["first"], count=case["count"])
    rec = norm_ref.fold_obs(norm_ref.new_record(10), case["obs"], **kw, **ra)
    rec, _ = norm_ref.fold_returns(rec, np.zeros((32, 3)), case["rew"], gamma=case["gamma"], **kw, **ra)
    xs, rs = _samples(case, windows)
    assert _miss(rec, xs, rs) <= 1.0
    no_ended = dict(ra, ended=np.zeros_like(case["ended"]))
    bad = norm_ref.fold_obs(norm_ref.new_record(10), case["obs"], **kw, **no_ended)
    bad, _ = norm_ref.fold_returns(bad, np.zeros((32, 3)), case["rew"], gamma=case["gamma"], **kw, **no_ended)
    assert bad["n_obs"] != rec["n_obs"]
    assert abs(bad["mean_ret"] - rs.mean()) > 1e4 * rs.size * 2.0 ** -52 * abs(rs.mean())
    # counting parked rows: every row of a learner in an env that was stepped
    L = case["T"] + 1
    sk = case["skip"] != 0
    valid = [np.broadcast_to(~sk[k % L][:, None] & (np.arange(3) < 2)[None, :], (32, 3)).reshape(-1)
             for k in range(case["first"], case["count"])]
    wrong = np.concatenate([case["obs"][k % L].reshape(-1, 10)[m].astype(np.float64)
                            for k, m in zip(range(case["first"], case["count"]), valid)])
    assert wrong.shape[0] > xs.shape[0]
    mean, var, _ = norm_ref.variances(rec)
    off = max(abs(mean[f] - wrong[:, f].mean()) / (xs.shape[0] * 2.0 ** -52 * np.abs(wrong[:, f]).mean()) for f in range(10))
    assert off > 1e4


@pytest.mark.parametrize("flags", ["rows", "packed"])
def test_the_sample_rule_is_ppos_weight(flags):
    """norm_ref.sample_mask against valid ∧ ¬_parked, computed by ppo.py's own expressions on CPU tensors."""
    from gym_uav_collision_avoidance_amd.ppo import PPO
    case = norm_layouts.ppo_ring()
    mem = norm_layouts.Ring(case, "cpu", packed_flags=flags == "packed")
    ppo = PPO(mem, generator=torch.Generator().manual_seed(1))
    steps = case["steps"]
    slots = ppo.advantages.window(steps)
    skip, _, _ = mem._flags(slots, slice(None))
    weight = (~skip).unsqueeze(-1)[:, :, :1].expand(-1, -1, mem.num_learners) & ~ppo._parked(slots, mem.count - steps)
    c = norm_layouts.packed(case) if flags == "packed" else case
    mine = np.stack([norm_ref.sample_mask(c["done"], k, c["learners"], c["skip"], c["ended"])
                     for k in range(case["first"], case["count"])])
    assert not mine[:, :, case["learners"]:].any()
    assert np.array_equal(mine[:, :, :case["learners"]], weight.numpy())
    assert 0 < int(weight.sum()) < weight.numel()
    # the planted rows: parked at k = 9 .. 13 in env 0, a sample again at k = 10 in env 1 and at k = 8 in env 2
    at = lambda k: mine[k - case["first"]]
    assert not at(9)[0, 0] and not at(13)[0, 0] and at(8)[0, 0] and at(10)[1, 1] and at(8)[2, 0] and not at(7)[2, 0]


# ---- the library -----------------------------------------------------------------------------------------------------------

def test_library_cross_compiles_and_carries_its_source_hash():
    x = _xlib()
    assert os.path.basename(x.LIB_PATH) == "libuavx_norm.so" and os.path.isfile(x.LIB_PATH)
    assert x.HEADER == os.path.join(ROOT, "include", "uavx_norm.h") and x.HEADER in x._sources()
    assert x._sources()[2] == os.path.join(ROOT, "include", "uavx_actor.h") and len(x._sources()) == 6
    assert x._sources()[3:] == [os.path.join(ROOT, PKG, "common_csrc", h)        # behind it, what the four small libraries share
                                for h in ("uavx_block_reduce.hpp", "uavx_entry.hpp", "uavx_ring_view.hpp")]
    assert any(f.endswith(os.path.join("norm_csrc", "uavx_norm.hip")) for f in x._sources())
    blob = open(x.LIB_PATH, "rb").read()
    assert f"UAVX_NORM_SRC_HASH={x.source_hash()}".encode() + b"\0" in blob and b"gfx950" in blob
    assert x._up_to_date()
    mk = open(os.path.join(x.CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, re.M).group(1)
    gae_mk = open(os.path.join(ROOT, PKG, "gae_csrc", "Makefile")).read()
    assert flags == re.search(r"^HIPFLAGS \?= (.*)$", gae_mk, re.M).group(1) and "-ffp-contract=off" in flags
    assert "UAVX_NORM_SRC_HASH" in mk and "OUT ?= libuavx_norm.so" in mk and "SRCHASH ?=" in mk
    assert "libuavx_norm.so.tmp*" in open(os.path.join(ROOT, ".gitignore")).read().split()


def test_library_exports_exactly_what_the_header_declares():
    x = _xlib()
    hdr = open(x.HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(uavx_norm_[a-z_0-9]*)\s*\(", code))
    assert declared == set(x.SYMBOLS) == set(x.FUNCTIONS) == {
        "uavx_norm_version", "uavx_norm_workspace_bytes", "uavx_norm_fold_obs", "uavx_norm_fold_returns", "uavx_norm_apply_obs",
        "uavx_norm_scale_rewards"}
    assert x.SYMBOLS[0] == "uavx_norm_version"
    lib = x.load()
    for name in sorted(declared):
        f = getattr(lib, name)
        assert (f.restype, list(f.argtypes)) == (x.FUNCTIONS[name][0], list(x.FUNCTIONS[name][1])), name
        # the header's parameter count is the table's
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, re.S).group(1)
        assert (0 if params.strip() == "void" else params.count(",") + 1) == len(x.FUNCTIONS[name][1]), name
    assert lib.uavx_norm_version() == x.ABI_VERSION == 1 and "#define UAVX_NORM_VERSION 1" in hdr
    assert f"#define UAVX_NORM_BLOCK {x.BLOCK}" in hdr and x.BLOCK == norm_ref.BLOCK
    assert f"#define UAVX_NORM_MAX_FEATURES {x.MAX_FEATURES}" in hdr and x.MAX_FEATURES == norm_ref.MAX_FEATURES
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", x.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l and "uavx" in l and not l.split()[-1].startswith("_Z")}
    assert exported == declared
    for cname, cls in (("uavx_norm_ring", x.Ring), ("uavx_norm_record", x.Record)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.search(r"(\w+)\s*(\[\w+\])?\s*$", d).group(1) for d in body.split(";") if d.strip()]
        assert fields == [n for n, _ in cls._fields_], cname
    assert ctypes.sizeof(x.Record) == x.RECORD_BYTES == 288 == 8 * norm_ref.words(norm_ref.new_record(10)).size
    assert ctypes.sizeof(x.Ring) == 64
    assert (x.Record.mean.offset, x.Record.M2.offset, x.Record.n_ret.offset, x.Record.M2_ret.offset) == (8, 136, 264, 280)


def test_bad_arguments_refused_before_any_device_call():
    x = _xlib()
    lib = x.load()
    bad, nan, inf = x.ERR_INVALID_ARG, float("nan"), float("inf")

    def ring(**kw):
        f = dict(rew=64, done=64, skip=64, ended=64, slots=6, envs=3, agents=2, learners=2)
        f.update(kw)
        return x.Ring(**f)

    def obs(r=None, obs=64, F=10, first=4, count=9, rec=64, work=64, work_bytes=1 << 20, **kw):
        r = ring(**kw) if r is None else r
        return lib.uavx_norm_fold_obs(ctypes.byref(r), obs, F, first, count, rec, work, work_bytes, None)

    def ret(r=None, first=4, count=9, gamma=0.99, carry=64, rec=64, work=64, work_bytes=1 << 20, **kw):
        r = ring(**kw) if r is None else r
        return lib.uavx_norm_fold_returns(ctypes.byref(r), first, count, gamma, carry, rec, work, work_bytes, None)

    # every refusal below comes before a launch: the addresses are not memory
    assert lib.uavx_norm_fold_obs(None, 64, 10, 4, 9, 64, 64, 1 << 20, None) == bad
    assert lib.uavx_norm_fold_returns(None, 4, 9, 0.99, 64, 64, 64, 1 << 20, None) == bad
    for call in (obs, ret):
        assert call(done=None) == bad and call(rec=None) == bad and call(work=None) == bad
        assert call(rec=68) == bad and call(work=68) == bad
        assert call(skip=None) == bad and call(ended=None) == bad             # only one of the two flag rows
        assert call(slots=1) == bad and call(slots=2 ** 31) == bad and call(envs=0) == bad and call(envs=2 ** 31) == bad
        assert call(agents=0) == bad and call(envs=2 ** 16, agents=2 ** 15) == bad
        assert call(learners=0) == bad and call(learners=3) == bad
        assert call(first=9) == bad and call(first=10) == bad                 # count − first = 0 and below
        assert call(first=3) == bad and call(first=0, count=6) == bad         # count − first = 6 > T = 5
        assert call(first=-1, count=3) == bad
        assert call(work_bytes=0) == bad and call(work_bytes=-8) == bad
    assert obs(obs=None) == bad and obs(obs=66) == bad
    assert obs(F=0) == bad and obs(F=17) == bad and obs(F=-1) == bad
    assert obs(work_bytes=8 * 21 - 1) == bad and obs(F=16, work_bytes=8 * 33 - 1) == bad
    assert obs(envs=129, work_bytes=2 * 8 * 21 - 1) == bad                    # 258 columns: two workgroups
    assert ret(rew=None) == bad and ret(rew=66) == bad and ret(carry=None) == bad and ret(carry=68) == bad
    assert ret(work_bytes=23) == bad
    for g in (-0.01, 1.01, nan, inf):
        assert ret(gamma=g) == bad, g

    def apply(rec=64, x_=64, out=64, rows=5, F=10, eps=1e-8, clip=10.0):
        return lib.uavx_norm_apply_obs(rec, x_, out, rows, F, eps, clip, None)

    def scale(rec=64, x_=64, out=64, count=5, eps=1e-8, clip=10.0):
        return lib.uavx_norm_scale_rewards(rec, x_, out, count, eps, clip, None)

    for call in (apply, scale):
        assert call(rec=None) == bad and call(x_=None) == bad and call(out=None) == bad
        assert call(rec=68) == bad and call(x_=66) == bad and call(out=66) == bad
        assert call(out=64 + 4) == bad and call(x_=64 + 16, out=64) == bad    # overlapping, but not the same
        for e in (-1e-8, nan, inf):
            assert call(eps=e) == bad, e
        for c in (0.0, -1.0, nan, inf):
            assert call(clip=c) == bad, c
    assert apply(F=0) == bad and apply(F=17) == bad and apply(rows=-1) == bad and apply(rows=2 ** 40) == bad
    assert scale(count=-1) == bad and scale(count=2 ** 40) == bad
    assert apply(rows=0) == x.OK and scale(count=0) == x.OK                   # nothing to do, nothing enqueued
    # the workspace: 8 · (2F + 1) bytes per 256 columns
    need = ctypes.c_int64(-1)
    for envs, agents, F, want in ((3, 2, 10, 168), (64, 4, 10, 168), (65, 4, 10, 336), (65536, 4, 10, 168 * 1024), (3, 2, 1, 24),
                                  (3, 2, 16, 264)):
        assert lib.uavx_norm_workspace_bytes(ctypes.byref(ring(envs=envs, agents=agents)), F, ctypes.byref(need)) == x.OK
        assert need.value == want, (envs, agents, F)
    assert lib.uavx_norm_workspace_bytes(None, 10, ctypes.byref(need)) == bad
    assert lib.uavx_norm_workspace_bytes(ctypes.byref(ring()), 10, None) == bad
    assert lib.uavx_norm_workspace_bytes(ctypes.byref(ring()), 0, ctypes.byref(need)) == bad
    assert lib.uavx_norm_workspace_bytes(ctypes.byref(ring()), 17, ctypes.byref(need)) == bad
    assert lib.uavx_norm_workspace_bytes(ctypes.byref(ring(envs=0)), 10, ctypes.byref(need)) == bad


def test_the_other_libraries_keep_their_hashes():
    import importlib
    from test_native_library_host import IDENTITY
    assert len(IDENTITY) == 7
    for name, (srchash, n) in IDENTITY.items():
        m = importlib.import_module(f"{PKG}.{name}")
        assert m.source_hash() == srchash and len(m._sources()) == n, name
        assert not any("norm" in os.path.basename(f) for f in m._sources()), name


def test_build_entry_builds_the_library():
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_norm_lib" in src.split("def smoke")[0]


# ---- what the Python layers do on the host ---------------------------------------------------------------------------------

def test_normalizer_arguments_refused_on_the_host():
    from gym_uav_collision_avoidance_amd import _norm_lib
    from gym_uav_collision_avoidance_amd.normalize import RolloutNormalizer
    was = _norm_lib.loaded()
    mem = norm_layouts.Ring(norm_layouts.make("count_9"), "cpu")
    for kw in (dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")), dict(gamma="0.9"), dict(gamma=True)):
        with pytest.raises(ValueError, match="must be a float in"):
            RolloutNormalizer(mem, **kw)
    for kw in (dict(clip_obs=0), dict(clip_reward=-1.0), dict(clip_obs=float("inf")), dict(clip_reward=True)):
        with pytest.raises(ValueError, match="must be a finite float > 0"):
            RolloutNormalizer(mem, **kw)
    for kw in (dict(eps=-1e-8), dict(eps=float("nan")), dict(eps="1e-8")):
        with pytest.raises(ValueError, match="must be a finite float >= 0"):
            RolloutNormalizer(mem, **kw)
    for kw in (dict(obs=1), dict(reward=None)):
        with pytest.raises(ValueError, match="must be a bool"):
            RolloutNormalizer(mem, **kw)
    norm = RolloutNormalizer(mem)
    assert norm.folded_obs == norm.folded_ret == 9 - 5 and norm.features == 10
    good = torch.zeros((4, 10))
    for x in (good.double(), torch.zeros((4, 9)), good.numpy(), None, torch.zeros(())):
        with pytest.raises(ValueError, match="observations must be float32"):
            norm.obs(x)
    with pytest.raises(ValueError, match="contiguous"):
        norm.obs(torch.zeros((10, 4)).t())
    for out in (good.double(), torch.zeros((3, 10)), torch.zeros((10, 4)).t()):
        with pytest.raises(ValueError, match="out must be"):
            norm.obs(good, out=out)
    for call in (lambda: norm.obs(good), norm.obs_ring, norm.rewards, norm.fold_obs, norm.fold_returns):
        with pytest.raises(ValueError, match="no CPU path"):
            call()
    mem.count = 9 - 5 + 6                                                    # six unfolded steps in a ring of T = 5
    for fold in (norm.fold_obs, norm.fold_returns):
        with pytest.raises(ValueError, match="overwritten"):
            fold()
    mem.count = 4
    norm.fold_obs(), norm.fold_returns()                                      # zero steps: a no-op, even without a device
    only_obs, only_rew = RolloutNormalizer(mem, reward=False), RolloutNormalizer(mem, obs=False)
    for call in (only_obs.rewards, only_obs.fold_returns, only_rew.obs_ring, only_rew.fold_obs, lambda: only_rew.obs(good)):
        with pytest.raises(ValueError, match="keeps no"):
            call()
    assert only_obs._rew_ring is None and only_rew._obs_ring is None
    st = norm.stats
    assert int(st.n_obs) == 0 and int(st.n_ret) == 0 and (st.var == 1).all() and float(st.var_ret) == 1.0
    assert _norm_lib.loaded() == was                                         # none of this needed the library
    # the state is plain data and loads under weights_only=True
    from gym_uav_collision_avoidance_amd.checkpoint import _plain
    norm.carry[1, 1], norm.folded_obs = 2.5, 3
    buf = io.BytesIO()
    torch.save(_plain(norm.state_dict(), "norm"), buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=True)
    other = RolloutNormalizer(mem).load_state_dict(sd)
    assert other.folded_obs == 3 and torch.equal(other.carry, norm.carry) and torch.equal(other._record, norm._record)
    for broken in ({"kind": "ppo"}, dict(sd, features=7), dict(sd, obs=False), dict(sd, record=sd["record"][:-1]),
                   dict(sd, carry=sd["carry"].float()), dict(sd, folded_ret=-1), dict(sd, folded_obs=True)):
        before = (other._record.clone(), other.carry.clone(), other.folded_obs, other.folded_ret)
        with pytest.raises(ValueError, match="uavx: "):
            other.load_state_dict(broken)
        assert torch.equal(before[0], other._record) and torch.equal(before[1], other.carry)
        assert before[2:] == (other.folded_obs, other.folded_ret)


def test_compute_rewards_refused_on_the_host():
    from gym_uav_collision_avoidance_amd import _gae_lib
    from gym_uav_collision_avoidance_amd.rollout import RolloutAdvantages
    was = _gae_lib.loaded()
    mem = gae_layouts.CraftedRing(gae_layouts.make("count_9"), "cpu")
    ra = RolloutAdvantages(mem)
    good = torch.zeros(ra.shape)
    for r in (good.double(), good[:-1], good.numpy(), 1.0):
        with pytest.raises(ValueError, match="rewards must be float32"):
            ra.compute(good, rewards=r)
    with pytest.raises(ValueError, match="rewards must be contiguous"):
        ra.compute(good, rewards=good.permute(2, 1, 0).contiguous().permute(2, 1, 0))
    with pytest.raises(ValueError, match="no CPU path"):
        ra.compute(good, rewards=good)
    assert _gae_lib.loaded() == was


def test_ppo_switches_refused_on_the_host_and_the_default_is_the_learner_as_it_was():
    from gym_uav_collision_avoidance_amd.ppo import PPO
    mem = norm_layouts.Ring(norm_layouts.make("count_9", 4, 2), "cpu")
    for kw in (dict(normalize_obs=1), dict(normalize_reward="yes"), dict(clip_obs=0), dict(clip_reward=float("nan")),
               dict(norm_eps=-1.0), dict(norm_eps=True)):
        with pytest.raises(ValueError, match="uavx: PPO: "):
            PPO(mem, **kw)
    held = {k: sys.modules.pop(k) for k in (f"{PKG}._norm_lib", f"{PKG}.normalize") if k in sys.modules}
    try:
        torch.manual_seed(3)
        ppo = PPO(mem, generator=torch.Generator().manual_seed(1))
        ppo.act()
        ppo.select_action(torch.zeros((3, 10)))
        sd = ppo.state_dict()
        assert f"{PKG}._norm_lib" not in sys.modules and f"{PKG}.normalize" not in sys.modules
    finally:
        sys.modules.update(held)
    assert set(sd) == {"kind", "policy", "value", "optimizer", "updates", "u", "logp"} and ppo.norm is None
    # a learner with a switch carries "norm"; neither loads the other's state, and nothing is written by the attempt
    torch.manual_seed(4)
    normed = PPO(mem, generator=torch.Generator().manual_seed(1), normalize_obs=True, normalize_reward=True)
    nsd = normed.state_dict()
    assert set(nsd) == set(sd) | {"norm"} and set(normed.state_dict(include_sampler=False)) == set(sd) - {"u", "logp"} | {"norm"}
    for learner, state, words in ((ppo, nsd, "with normalisation, this one is built without"),
                                  (normed, sd, "without normalisation, this one is built with")):
        before = [p.clone() for p in learner.params]
        with pytest.raises(ValueError, match=words):
            learner.load_state_dict(state)
        assert all(torch.equal(a, b) for a, b in zip(before, learner.params))
    only_obs = PPO(mem, generator=torch.Generator().manual_seed(1), normalize_obs=True)
    before = [p.clone() for p in only_obs.params]
    with pytest.raises(ValueError, match="reward = True"):
        only_obs.load_state_dict(nsd)
    assert all(torch.equal(a, b) for a, b in zip(before, only_obs.params))
    with pytest.raises(ValueError, match="no CPU path"):
        normed.act()

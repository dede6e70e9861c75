"""Host-side checks of GAE(λ) over the ring (libuavx_gae.so, include/uavx_gae.h): the numpy restatement the
GPU tests trust (gae_ref.py) equals a second, per-column writing of the header's prose bit for bit on every crafted layout,
agrees with the textbook special cases (λ = 0: the one-step TD error; λ = 1 without cuts: the discounted return) and its
documented summation order with numpy's two-pass standard deviation; the two writings also agree on the row-group windows,
the straddled shapes and past 256 partials (the shapes of test_gpu_gae.py), and the restatement is held to the definition of
GAE(λ) itself, the forward view summed in exact rational arithmetic (gae_forward.py), within a derived bound; the library builds for gfx950 without a GPU, carries
its source hash, exports exactly what its header declares and refuses every bad argument before touching a device; the other
libraries keep their pinned hashes; the Python layer refuses bad arguments on the host and a PPO's state is plain data."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

import gae_layouts
import gae_ref
from gae_ref import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _xlib():
    from gym_uav_collision_avoidance_amd import _gae_lib
    _gae_lib.build()
    return _gae_lib


# ---- the restatement -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", ["rows", "packed"])
@pytest.mark.parametrize("name", sorted(gae_layouts.LAYOUTS))
def test_restatement_equals_the_loop_bit_for_bit(name, flags):
    case = gae_layouts.make(name)
    case = gae_layouts.packed(case) if flags == "packed" else case
    kw = gae_layouts.ref_args(case)
    adv, ret, valid = gae_ref.gae(fill=7, **kw)
    adv2, ret2, valid2 = gae_ref.gae_loop(fill=7, **kw)
    assert same(adv, adv2) and same(ret, ret2) and same(valid, valid2)
    st, st2 = gae_ref.stats(adv, valid, case["count"], case["steps"]), gae_ref.stats_loop(adv, valid, case["count"], case["steps"])
    assert st[0] == st2[0] and same(np.float64(st[1:]), np.float64(st2[1:])), (st, st2)
    # rows outside the window keep the fill, rows inside never do
    inside = np.zeros(adv.shape[0], bool)
    inside[gae_ref.window_slots(case["count"], case["steps"], adv.shape[0])] = True
    assert np.all(valid[~inside] == 7) and np.all(adv[~inside] == 7) and np.all(valid[inside] <= 1)
    assert int(inside.sum()) == case["steps"]


def test_layouts_hold_what_their_names_say():
    g = lambda name: gae_layouts.make(name)
    run = lambda c: gae_ref.gae(**gae_layouts.ref_args(c))
    c = g("all_skip")
    adv, ret, valid = run(c)
    norm, st = gae_ref.normalise(adv, valid, c["count"], c["steps"])
    assert st == (0, 0.0, 0.0) and not valid.any() and not np.isnan(norm).any() and not norm.any()
    c = g("one_valid_entry")
    adv, ret, valid = run(c)
    norm, st = gae_ref.normalise(adv, valid, c["count"], c["steps"])
    assert st[0] == 1 and st[2] == 0.0 and int(valid.sum()) == 1 and st[1] == float(adv[valid == 1][0])
    assert not norm.any() and not np.isnan(norm).any()
    c = g("nan_not_bootstrapped")
    assert np.isnan(c["values"]).sum() >= 2
    adv, ret, valid = run(c)
    assert not np.isnan(adv).any() and not np.isnan(ret).any()
    c = g("nan_bootstrapped")
    adv, ret, valid = run(c)
    L = c["T"] + 1
    assert np.isnan(adv[(c["count"] - 1) % L, 0, 0]) and np.isnan(adv[7 % L, 0, 0])
    assert not np.isnan(adv[6 % L]).any() and np.isnan(adv).sum() == 2       # the ended row at k = 6 stops it
    c = g("fewer_learners")
    adv, ret, valid = run(c)
    assert c["learners"] < c["N"] and not valid[:, :, c["learners"]:].any() and valid[:, :, :c["learners"]].any()
    c = g("large_mean")
    adv, ret, valid = run(c)
    n, mean, std = gae_ref.stats(adv, valid, c["count"], c["steps"])
    assert 3e3 <= abs(mean) / std <= 3e4
    c = g("negative_zero_rewards")
    assert np.signbit(c["rew"]).all()
    for name, count in (("count_3", 3), ("count_5", 5), ("count_9", 9), ("count_13", 13)):
        assert g(name)["count"] == count and g(name)["T"] == 5
    assert [g(f"steps_{s}")["steps"] for s in ("1", "2", "T")] == [1, 2, 5]
    p = gae_layouts.packed(g("count_9"))
    assert p["skip"] is None and (p["done"][:, :, 0] & 8).any()              # "truncated" rides along and is ignored


def test_lambda_zero_is_the_one_step_td_error():
    c = gae_layouts.big(5, 3, 9, seed=81)
    c["lam"] = 0.0
    adv, ret, valid = gae_ref.gae(**gae_layouts.ref_args(c))
    L = c["T"] + 1
    for k in range(c["count"] - c["steps"], c["count"]):
        s, s1 = k % L, (k + 1) % L
        live = 1.0 - (c["done"][s] & 1).astype(np.float64)
        td = (c["rew"][s].astype(np.float64) + c["gamma"] * c["values"][s1].astype(np.float64) * live) - c["values"][s]
        ok = valid[s] == 1
        assert ok.any() and same(adv[s][ok], td.astype(np.float32)[ok])


def test_lambda_one_without_cuts_is_the_discounted_return():
    c = gae_layouts._clean(4, 2, T=12, count=30, seed=82, gamma=0.97, lam=1.0)
    adv, ret, valid = gae_ref.gae(**gae_layouts.ref_args(c))
    L, count, g = c["T"] + 1, c["count"], c["gamma"]
    assert valid[gae_ref.window_slots(count, c["steps"], L)].all()
    for k in range(count - c["steps"], count):
        direct = sum(g ** (j - k) * c["rew"][j % L].astype(np.float64) for j in range(k, count))
        direct = direct + g ** (count - k) * c["values"][count % L].astype(np.float64)
        # ret is the float32 rounding (2^-24 relative) of a float64 sum that differs from `direct` by a few 1e-16 per term
        assert np.all(np.abs(ret[k % L] - direct) <= 2.0 ** -24 * np.abs(direct) + 1e-12), k


@pytest.mark.parametrize("case", ["big", "large_mean", "three_workgroups"])
def test_documented_summation_order_against_numpy_two_pass_std(case):
    c = {"big": lambda: gae_layouts.big(70, 4, 8, learners=3),
         "large_mean": lambda: gae_layouts.make("large_mean", 40, 4),
         "three_workgroups": lambda: gae_layouts.big(160, 4, 6, seed=83)}[case]()
    adv, ret, valid = gae_ref.gae(**gae_layouts.ref_args(c))
    n, mean, std = gae_ref.stats(adv, valid, c["count"], c["steps"])
    slots = gae_ref.window_slots(c["count"], c["steps"], adv.shape[0])
    a = adv[slots][valid[slots] == 1].astype(np.float64)
    assert n == a.size and n > 100
    want = np.std(a, ddof=1)
    bound = n * 2.0 ** -52
    print(f"{case}: n = {n}, std = {std!r}, numpy = {want!r}, relative difference {abs(std - want) / want:.3e}, bound {bound:.3e}")
    assert abs(std - want) <= bound * want
    assert abs(mean - a.mean()) <= bound * max(abs(a.mean()), np.abs(a).mean())


# ---- windows around the groups of rows the walk fetches together -------------------------------------------------------------

def _restatement_equals_the_loop(case):
    kw = gae_layouts.ref_args(case)
    adv, ret, valid = gae_ref.gae(fill=7, **kw)
    adv2, ret2, valid2 = gae_ref.gae_loop(fill=7, **kw)
    assert same(adv, adv2) and same(ret, ret2) and same(valid, valid2)
    st, st2 = gae_ref.stats(adv, valid, case["count"], case["steps"]), gae_ref.stats_loop(adv, valid, case["count"], case["steps"])
    assert st[0] == st2[0] > 0 and same(np.float64(st[1:]), np.float64(st2[1:])), (st, st2)


@pytest.mark.parametrize("flags", ["rows", "packed"])
@pytest.mark.parametrize("wrapped", [True, False], ids=["count40", "count_steps"])
@pytest.mark.parametrize("steps", gae_layouts.GROUP_STEPS)
def test_restatement_equals_the_loop_around_the_row_groups(steps, wrapped, flags):
    case = gae_layouts.row_groups(steps, wrapped)
    _restatement_equals_the_loop(gae_layouts.packed(case) if flags == "packed" else case)


@pytest.mark.parametrize("flags", ["rows", "packed"])
@pytest.mark.parametrize("shape", [(300, 1, None), (100, 3, None), (60, 5, 3), (40, 7, 1)], ids=["300x1", "100x3", "60x5_l3", "40x7_l1"])
def test_restatement_equals_the_loop_with_envs_across_wavefront_edges(shape, flags):
    case = gae_layouts.big(shape[0], shape[1], 12, learners=shape[2], seed=73)
    _restatement_equals_the_loop(gae_layouts.packed(case) if flags == "packed" else case)


def test_row_group_layout_holds_what_its_docstring_says():
    R = gae_layouts.ROWS
    assert R == 8 and gae_layouts.T_GROUPS == 24 and gae_layouts.GROUP_STEPS == (7, 8, 9, 15, 16, 17, 23, 24)
    for wrapped in (True, False):
        c = gae_layouts.row_groups(24, wrapped)
        assert (c["T"], c["E"], c["N"], c["learners"], c["steps"], c["count"]) == (24, 100, 3, 2, 24, 40 if wrapped else 24)
        L = c["T"] + 1
        row = lambda name, j: c[name][(c["count"] - 1 - j) % L]               # the row at walk position j
        skips = {e: [j for j in range(24) if row("skip", j)[e]] for e in range(8)}
        assert skips == {0: [7], 1: [8], 2: [7, 8], 3: [], 4: [], 5: [], 6: [], 7: [6]}
        assert {e: [j for j in range(24) if row("ended", j)[e]] for e in range(8)} == {e: [8] if e == 3 else [] for e in range(8)}
        dones = {(e, i): [j for j in range(24) if row("done", j)[e, i]] for e in range(8) for i in range(3)}
        assert {q: js for q, js in dones.items() if js} == {(4, 0): [15], (5, 1): [16], (6, 0): list(range(8, 17))}
        assert c["skip"][:, 8:].any() and c["ended"][:, 8:].any() and c["done"][:, 8:].any()      # the low-rate rest
        assert 0.005 < c["skip"][:, 8:].mean() < 0.08
        adv, ret, valid = gae_ref.gae(**gae_layouts.ref_args(c))
        # what the events do to the walk: a skip row cuts the row before it and restarts the carry after it
        s7, s8, s9 = [(c["count"] - 1 - j) % L for j in (7, 8, 9)]
        assert not valid[s7, 0].any() and valid[s8, 0, :2].all() and not valid[s8, 1].any() and valid[s9, 1, :2].all()
        assert not valid[s7, 2].any() and not valid[s8, 2].any() and not valid[:, :, 2].any()
        td = lambda s, e, i: np.float32((float(c["rew"][s, e, i]) + c["gamma"] * float(c["values"][(s + 1) % L, e, i]))
                                        - float(c["values"][s, e, i]))
        assert adv[s8, 0, 0] == td(s8, 0, 0) and adv[s9, 1, 0] == td(s9, 1, 0) and adv[s8, 3, 1] == td(s8, 3, 1)
        assert adv[s7, 3, 1] != td(s7, 3, 1) and adv[s8, 7, 0] != td(s8, 7, 0)    # an uncut row is more than its TD error
    # count = steps: the events before step 0 are not planted, the others are where they were
    c = gae_layouts.row_groups(9, False)
    assert c["count"] == 9 and c["skip"][1, 0] and c["skip"][0, 1] and c["skip"][[0, 1], 2].all() and c["ended"][0, 3]
    assert c["skip"][2, 7] and int(c["skip"][:, :8].sum()) == 5
    assert not c["done"][:, :4].any() and c["done"][0, 6, 0] and int(c["done"][:, :8].sum()) == 1
    c = gae_layouts.row_groups(7, False)
    assert c["skip"][0, 7] and int(c["skip"][:, :8].sum()) == 1 and not c["ended"][:, :8].any() and not c["done"][:, :8].any()


@pytest.mark.parametrize("shape", [(16385, 4, 257), (43691, 3, 513)], ids=["257_partials", "513_partials"])
def test_summation_order_equals_the_loop_past_256_partials(shape):
    """The geometry of the two largest GPU cases, reduced to one step and a few hundred valid entries: thread t of the last
    sum adds partials t, t + 256 (and t + 512); the last workgroup holds 4 columns (1 column)."""
    E, N, blocks = shape
    cols = E * N
    assert -(-cols // gae_ref.BLOCK) == blocks > gae_ref.BLOCK
    rng = np.random.default_rng(blocks)
    adv = np.zeros((2, E, N), np.float32)
    valid = np.zeros((2, E, N), np.uint8)
    pick = np.unique(np.concatenate([rng.choice(cols, 600, replace=False),
                                     [0, 255, 256, 256 * 256, 256 * 256 + 1, 512 * 256 if blocks > 512 else 0, cols - 1]]))
    valid[0].reshape(-1)[pick] = 1
    adv[0].reshape(-1)[pick] = (rng.normal(size=pick.size) * 10.0 ** rng.integers(-3, 4, pick.size)).astype(np.float32)
    adv[1] = 9.0                                                              # outside the window
    touched = {int(q) // gae_ref.BLOCK for q in pick}
    assert {0, 256, blocks - 1} <= touched and any(b % 256 == b2 % 256 and b != b2 for b in touched for b2 in touched)
    st, st2 = gae_ref.stats(adv, valid, 1, 1), gae_ref.stats_loop(adv, valid, 1, 1)
    assert st[0] == st2[0] == pick.size and same(np.float64(st[1:]), np.float64(st2[1:])), (st, st2)
    want = adv[0][valid[0] == 1].astype(np.float64)
    assert abs(st[1] - want.mean()) <= pick.size * 2.0 ** -52 * np.abs(want).mean()
    assert abs(st[2] - np.std(want, ddof=1)) <= pick.size * 2.0 ** -52 * np.std(want, ddof=1)


# ---- the definition itself ---------------------------------------------------------------------------------------------------

def _against_the_definition(case):
    """gae_ref.gae's adv and ret against the forward view in exact arithmetic:
        |got − exact| <= 2^-24·|exact| + steps·2^-50·M + 2^-149
    One float32 rounding of the result; at most eight float64 roundings per row of the recurrence (the casts are exact; γ·V, r
    + b, − V, γλ·A⁺, + δ, and for ret + V; γλ itself is one rounded product), each at most 2^-53 of a quantity bounded by M,
    the same sum over absolute values, accumulated over at most `steps` rows: steps · 8 · 2^-53 · M; the subnormal floor."""
    import gae_forward
    from fractions import Fraction
    kw = gae_layouts.ref_args(case)
    adv, ret, valid = gae_ref.gae(**kw)
    exact = gae_forward.forward_view(**kw)
    L, steps = case["T"] + 1, case["steps"]
    sk, _ = gae_ref.flag_rows(case["done"], case["skip"], case["ended"])
    slots = gae_ref.window_slots(case["count"], steps, L)
    assert not valid[slots][sk[slots]].any()                                  # skip rows are not entries
    keys = {(k, e, i) for k in range(case["count"] - steps, case["count"]) for e in range(case["E"]) for i in range(case["N"])
            if valid[k % L, e, i]}
    assert keys == set(exact) and len(keys) > 0
    worst, lengths = 0.0, set()
    for (k, e, i), (A, R, M, MR) in exact.items():
        for got, want, scale in ((adv[k % L, e, i], A, M), (ret[k % L, e, i], R, MR)):
            bound = Fraction(1, 2 ** 24) * abs(want) + steps * Fraction(1, 2 ** 50) * scale + Fraction(1, 2 ** 149)
            err = abs(Fraction(float(got)) - want)
            worst = max(worst, float(err / bound))
            assert err <= bound, (k, e, i, float(got), float(want), float(err), float(bound))
    return worst, len(keys)


@pytest.mark.parametrize("name", ["seed1", "seed2", "seed3", "gamma1_lambda1", "one_learner", "packed"])
def test_restatement_against_the_definition_in_exact_arithmetic(name):
    kw = dict(T=20, count=33, steps=20, gamma=0.99, lam=0.95)
    case = {"seed1": lambda: gae_layouts._base(4, 2, seed=91, **kw),
            "seed2": lambda: gae_layouts._base(4, 2, seed=92, **kw),
            "seed3": lambda: gae_layouts._base(4, 2, seed=93, **kw),
            "gamma1_lambda1": lambda: gae_layouts._base(4, 2, seed=94, **dict(kw, gamma=1.0, lam=1.0)),
            "one_learner": lambda: gae_layouts._base(4, 2, seed=95, learners=1, **kw),
            "packed": lambda: gae_layouts.packed(gae_layouts._base(4, 2, seed=96, **kw))}[name]()
    flags = gae_ref.flag_rows(case["done"], case["skip"], case["ended"])
    assert (case["done"] & 1).any() and flags[0].any() and flags[1].any()
    worst, n = _against_the_definition(case)
    print(f"{name}: {n} entries, worst |got - exact| / bound = {worst:.3f}")


def test_the_definition_sees_a_wrong_recurrence():
    """The forward view has teeth: a restatement that bootstrapped through an agent's done, or let the carry pass a skip row,
    would miss the bound by orders of magnitude."""
    import gae_forward
    from fractions import Fraction
    case = gae_layouts._base(4, 2, T=20, count=33, steps=20, seed=91)
    kw = gae_layouts.ref_args(case)
    adv, ret, valid = gae_ref.gae(**kw)
    exact = gae_forward.forward_view(**kw)
    for wrong in (dict(kw, done=np.zeros_like(case["done"])), dict(kw, skip=np.zeros_like(case["skip"]))):
        bad, _, _ = gae_ref.gae(**wrong)
        off = [abs(Fraction(float(bad[k % 21, e, i])) - A) / (Fraction(1, 2 ** 24) * abs(A) + 20 * Fraction(1, 2 ** 50) * M)
               for (k, e, i), (A, _, M, _) in exact.items() if abs(A) > 0]
        assert max(off) > 1e4


# ---- the library -----------------------------------------------------------------------------------------------------------

def test_library_cross_compiles_and_carries_its_source_hash():
    x = _xlib()
    assert os.path.basename(x.LIB_PATH) == "libuavx_gae.so" and os.path.isfile(x.LIB_PATH)
    assert x.HEADER == os.path.join(ROOT, "include", "uavx_gae.h") and x.HEADER in x._sources()
    assert any(f.endswith(os.path.join("gae_csrc", "uavx_gae.hip")) for f in x._sources())
    blob = open(x.LIB_PATH, "rb").read()
    assert f"UAVX_GAE_SRC_HASH={x.source_hash()}".encode() + b"\0" in blob and b"gfx950" in blob
    assert x._up_to_date()
    mk = open(os.path.join(x.CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, re.M).group(1)
    actor_mk = open(os.path.join(ROOT, "gym_uav_collision_avoidance_amd", "actor_csrc", "Makefile")).read()
    assert flags == re.search(r"^HIPFLAGS \?= (.*)$", actor_mk, re.M).group(1) and "-ffp-contract=off" in flags
    assert "UAVX_GAE_SRC_HASH" in mk and "OUT ?= libuavx_gae.so" in mk and "SRCHASH ?=" in mk
    assert "libuavx_gae.so.tmp*" in open(os.path.join(ROOT, ".gitignore")).read().split()


def test_library_exports_exactly_what_the_header_declares():
    x = _xlib()
    hdr = open(x.HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(uavx_gae_[a-z_0-9]*)\s*\(", code))
    assert declared == set(x.SYMBOLS) == set(x.FUNCTIONS) == {"uavx_gae_version", "uavx_gae_workspace_bytes",
                                                              "uavx_gae_compute"}
    assert x.SYMBOLS[0] == "uavx_gae_version"
    lib = x.load()
    for name in sorted(declared):
        f = getattr(lib, name)
        assert (f.restype, list(f.argtypes)) == (x.FUNCTIONS[name][0], list(x.FUNCTIONS[name][1])), name
    assert lib.uavx_gae_version() == x.ABI_VERSION == 1 and "#define UAVX_GAE_VERSION 1" in hdr
    assert f"#define UAVX_GAE_BLOCK {x.BLOCK}" in hdr and x.BLOCK == gae_ref.BLOCK
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", x.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l and "uavx" in l and not l.split()[-1].startswith("_Z")}
    assert exported == declared
    for cname, cls in (("uavx_gae_ring", x.Ring), ("uavx_gae_stats", x.Stats)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.search(r"(\w+)\s*$", d).group(1) for d in body.split(";") if d.strip()]
        assert fields == [n for n, _ in cls._fields_], cname
    assert ctypes.sizeof(x.Stats) == x.STATS_BYTES == 24 and ctypes.sizeof(x.Ring) == 64


def test_bad_arguments_refused_before_any_device_call():
    x = _xlib()
    lib = x.load()
    bad, nan = x.ERR_INVALID_ARG, float("nan")

    def ring(**kw):
        f = dict(rew=64, done=64, skip=64, ended=64, slots=6, envs=3, agents=2, learners=2)
        f.update(kw)
        return x.Ring(**f)

    def call(r=None, values=64, count=9, steps=5, gamma=0.99, lam=0.95, adv=64, ret=64, valid=64, norm=64, stats=64, work=64,
             work_bytes=1 << 20, **kw):
        r = ring(**kw) if r is None else r
        return lib.uavx_gae_compute(ctypes.byref(r), values, count, steps, gamma, lam, adv, ret, valid, norm, stats, work,
                                    work_bytes, None)

    # every refusal below comes before a launch: the addresses are not memory
    assert lib.uavx_gae_compute(None, 64, 9, 5, 0.99, 0.95, 64, 64, 64, 64, 64, 64, 1 << 20, None) == bad
    for name in ("rew", "done"):
        assert call(**{name: None}) == bad, name
    for name in ("values", "adv", "ret", "valid"):
        assert call(**{name: None}) == bad, name
    assert call(rew=66) == bad and call(values=66) == bad and call(adv=66) == bad and call(ret=66) == bad and call(norm=66) == bad
    assert call(slots=1) == bad and call(slots=0) == bad and call(slots=2 ** 31) == bad
    assert call(envs=0) == bad and call(envs=-1) == bad and call(envs=2 ** 31) == bad
    assert call(agents=0) == bad and call(agents=2 ** 31) == bad and call(envs=2 ** 16, agents=2 ** 15) == bad
    assert call(learners=0) == bad and call(learners=3) == bad and call(learners=-1) == bad
    assert call(count=0) == bad and call(count=-3) == bad
    assert call(steps=0) == bad and call(steps=-1) == bad and call(steps=6) == bad and call(count=3, steps=4) == bad
    for g in (-0.01, 1.01, nan, float("inf")):
        assert call(gamma=g) == bad and call(lam=g) == bad, g
    assert call(skip=None) == bad and call(ended=None) == bad                 # only one of the two flag rows
    assert call(stats=None) == bad and call(work=None) == bad                 # adv_norm without its record or workspace
    assert call(stats=68) == bad and call(work=68) == bad
    assert call(work_bytes=23) == bad and call(work_bytes=0) == bad and call(work_bytes=-24) == bad
    assert call(envs=129, work_bytes=47) == bad                               # 258 columns: two workgroups
    # the workspace: 24 bytes per 256 columns
    need = ctypes.c_int64(-1)
    for envs, agents, want in ((3, 2, 24), (64, 4, 24), (65, 4, 48), (65536, 4, 24 * 1024), (2 ** 29, 3, 24 * 6291456)):
        assert lib.uavx_gae_workspace_bytes(ctypes.byref(ring(envs=envs, agents=agents)), ctypes.byref(need)) == x.OK
        assert need.value == want, (envs, agents)
    assert lib.uavx_gae_workspace_bytes(None, ctypes.byref(need)) == bad
    assert lib.uavx_gae_workspace_bytes(ctypes.byref(ring()), None) == bad
    assert lib.uavx_gae_workspace_bytes(ctypes.byref(ring(envs=0)), ctypes.byref(need)) == bad
    assert lib.uavx_gae_workspace_bytes(ctypes.byref(ring(envs=2 ** 16, agents=2 ** 15)), ctypes.byref(need)) == bad


def test_the_other_libraries_keep_their_hashes():
    from gym_uav_collision_avoidance_amd import _actor_lib, _lib, _prio_lib
    assert _actor_lib.source_hash() == "c6725b15f59f1983"        # 17c0e2c29cadcdb4 before its replay unit took the ring's view and the n-step walk from common_csrc/
    assert _prio_lib.source_hash() == "75c3f7d1033d0f00"         # 3e2046d3591a64b0 before it took the ring's view and the entry plumbing from common_csrc/
    assert _lib.source_hash() == "c85b3516db0d8e1b"
    for mod in (_actor_lib, _prio_lib, _lib):
        assert not any("gae" in os.path.basename(f) for f in mod._sources())


# ---- what the Python layer does on the host --------------------------------------------------------------------------------

def test_rollout_arguments_refused_on_the_host():
    from gym_uav_collision_avoidance_amd import _gae_lib
    from gym_uav_collision_avoidance_amd.rollout import RolloutAdvantages
    was = _gae_lib.loaded()
    mem = gae_layouts.CraftedRing(gae_layouts.make("count_9"), "cpu")
    for kw in (dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")), dict(lam=2), dict(lam="0.9"), dict(gamma=True)):
        with pytest.raises(ValueError, match="must be a float in"):
            RolloutAdvantages(mem, **kw)
    ra = RolloutAdvantages(mem)
    good = torch.zeros(ra.shape)
    for steps in (0, -1, 6, 2.0, True):
        with pytest.raises(ValueError, match="steps must be an int"):
            ra.compute(good, steps)
    for v in (good.double(), good[:-1], good.numpy(), None):
        with pytest.raises(ValueError, match="values must be float32"):
            ra.compute(v)
    with pytest.raises(ValueError, match="contiguous"):
        ra.compute(good.permute(2, 1, 0).contiguous().permute(2, 1, 0))
    with pytest.raises(ValueError, match="no CPU path"):
        ra.compute(good)
    mem.count = 0
    with pytest.raises(ValueError, match="holds no step"):
        ra.compute(good)
    assert _gae_lib.loaded() == was                                          # none of this needed the library
    mem.count = 9
    assert ra.window().tolist() == [4, 5, 0, 1, 2] and ra.window(2).tolist() == [1, 2]
    mem.count = 3
    assert ra.window().tolist() == [0, 1, 2]


def test_ppo_state_is_plain_data_and_bad_arguments_are_refused():
    from gym_uav_collision_avoidance_amd.checkpoint import _plain
    from gym_uav_collision_avoidance_amd.ppo import PPO
    mem = gae_layouts.CraftedRing(gae_layouts.make("count_9", 4, 2), "cpu")
    torch.manual_seed(3)
    ppo = PPO(mem, generator=torch.Generator().manual_seed(1))
    ppo.act()
    assert float(mem.action_slot().abs().max()) <= 1.0 and float(ppo.logp[mem.count % mem.L].abs().sum()) > 0
    buf = io.BytesIO()
    torch.save(_plain(ppo.state_dict(), "agent"), buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=True)
    torch.manual_seed(4)
    other = PPO(mem, generator=torch.Generator().manual_seed(1))
    assert not torch.equal(other.policy.linear1.weight, ppo.policy.linear1.weight)
    other.load_state_dict(sd)
    for a, b in zip(ppo.params, other.params):
        assert torch.equal(a, b)
    assert torch.equal(other.u, ppo.u) and torch.equal(other.logp, ppo.logp)
    assert "u" not in ppo.state_dict(include_sampler=False)
    with pytest.raises(ValueError, match="another learner"):
        other.load_state_dict({"kind": "sac"})
    for kw in (dict(lr=0), dict(clip=-0.1), dict(epochs=0), dict(minibatches=1.5), dict(vf_coef=-1), dict(ent_coef=float("nan")),
               dict(max_grad_norm=0), dict(rollout=6), dict(rollout=0), dict(minibatches=7), dict(gamma=1.5)):
        with pytest.raises(ValueError, match="uavx: "):
            PPO(mem, **kw)

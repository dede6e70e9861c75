"""What the crafted batches of tests/threshold_layouts.py hold, proved on the CPU (host model against the oracle), so that
tests/test_gpu_threshold_edges.py is known to stand ON every threshold of the step kernels:
  1. the oracle's post-step quantity of every ego (square to its neighbour, prev_distance, velocity, position) is bit-equal to
     the host model's: the member sits exactly where its tag says;
  2. within every class the oracle's decision is the one the member's tag names (it flips between the two named members and
     nowhere else), in reward, collision counter, done bit and DONE / COLLIDED flags;
  3. where the decision shows in the reward the two sides differ by >= 0.5, ten thousand times the 1e-5 the GPU test allows;
  4. N = 4: threshold egos sit in wavefronts on the fast path of scan_neighbours_sq and in wavefronts pulled into its fallback;
  5. N = 7, 8, 13, 24: threshold egos sit in wavefronts with 0, with 1-6 and with >= 7 near-tie lanes (the key scan's exits);
  6. every class and every member occurs in every batch; nothing is masked or drawn at test time.
The reference's own verdict on the same thresholds (tests/golden/live_thresholds.npz, recorded from the reference by
tests/golden/make_live_golden.py thresholds) pins the oracle there, bit for bit, reward included."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import neighbour_layouts as nl  # noqa: E402
import threshold_layouts as tl  # noqa: E402
from golden_util import load_fixture  # noqa: E402
from make_live_golden import thr_groups  # noqa: E402
from threshold_layouts import F32, bits, nxt  # noqa: E402

AGENTS = (1, 2, 3, 4, 5, 7, 8, 13, 24)
CASES = [(n, w, c) for n in AGENTS for w in tl.WORLDS for c in ("f64", "f32") if tl.classes_of(n, w)]
IN_REWARD = ("C", "Ct", "CS", "GS", "G", "S")
DONE, COLLIDED = 1, 2


def expected_members(n, world):
    """(cls, member) of every ego a batch must hold, spelt out independently of the generator's loops."""
    out = []
    both = ("/below", "/above")
    for cls in tl.classes_of(n, world):
        if cls in ("C", "Ct", "H"):
            out += [(cls, m + o) for m in ("L-1", "L", "L+1", "2R^2") for o in both]
        elif cls == "CS":
            out += [(cls, m + o) for m in ("sense-1", "sense", "sense+1") for o in both]
        elif cls == "GS":
            out += [(cls, m + o) for m in ("L+1>L", "L>L+1") for o in both]
        elif cls == "G":
            out += [(cls, f"{k}/{m}") for k in ("axis", "diag") for m in ("0.5-1", "0.5", "0.5+1")]
            out += [(cls, "blocked/0.5-1")] if n >= 2 else []
        elif cls == "S":
            out += [(cls, m) for m in ("1c/below", "1c/at", "1c/above", "2c/lim-1", "2c/lim", "2c/lim+1")]
        elif cls == "O":
            out += [(cls, f"{a}-{s}/{m}/{k}") for a in "xy" for s in ("hi", "lo") for m in ("in", "out") for k in ("still", "coast")]
        elif cls == "V":
            out += [(cls, f"{k}/{a}{s}/{u}") for k in ("acc", "vel") for a in "xy" for s in "+-" for u in (0, 1)]
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------------------
# the host model itself
def test_sq_limit_le_is_the_square_plus_one_ulp_at_the_usual_radii():
    for lim in (0.5, 0.6, 0.9, 1.0, 1.4, 2.0):
        f = F32(lim)
        L = tl.sq_limit_le(lim)
        assert int(bits(L)) - int(bits(F32(f * f))) == 1, lim           # the naive limit lim*lim is one float32 step short
        assert np.sqrt(L) <= f < np.sqrt(nxt(L, 1))
    assert int(bits(nl.sq_limit_lt(1.4))) - int(bits(F32(F32(1.4) * F32(1.4)))) == -1
    for lim in (0.5, 0.6, 0.9, 1.0, 2.0, 1.8, 3.0):
        assert nl.sq_limit_lt(lim) == F32(F32(lim) * F32(lim)), lim


def test_box_limits_and_speed_limit():
    assert tl.f32_at_or_below(25.0) == F32(25.0) == tl.f32_at_or_above(25.0)
    nearest_outside = []
    for half in (6.15, 4.85):                                           # the halves of the 12.3 x 9.7 box
        lo, hi = tl.f32_at_or_above(-half), tl.f32_at_or_below(half)
        assert float(hi) <= half < float(nxt(hi, 1)) and float(nxt(lo, -1)) < -half <= float(lo)
        nearest_outside.append(F32(half) != hi and F32(-half) != lo)
    assert nearest_outside == [True, False]     # f32(6.15) > 6.15: a plain cast of the x half lets one float32 too many in
    s = tl.SPEED_SQ_LIM
    assert math.sqrt(s) >= 0.2 > math.sqrt(float(nxt(s, -1)))
    if hasattr(math, "fma"):
        assert tl.speed_sq(0.12, 0.16) == math.fma(0.16, 0.16, 0.12 * 0.12)


def test_generator_is_deterministic():
    tl._cache.clear()
    a = tl.make_threshold_batch(7, "r03")
    tl._cache.clear()
    b = tl.make_threshold_batch(7, "r03")
    for k in ("loc", "vel", "act", "tgt", "prev_d", "init_d"):
        assert np.array_equal(a[k], b[k]), k
    assert [(g["env"], g["agent"], g["cls"], g["member"]) for g in a["egos"]] == \
           [(g["env"], g["agent"], g["cls"], g["member"]) for g in b["egos"]]


# ---------------------------------------------------------------------------------------------------------------------------
def _stepped(oracle_mod, b):
    """The oracle stepped twice on the batch: per step (obs, rew, done, state), and the oracle."""
    orc = tl.oracle_for(oracle_mod, b)
    out = []
    for _ in range(2):
        o, r, d = orc.step(b["act"])
        out.append(dict(rew=r.copy(), done=d.copy(), loc=orc.loc.astype(F32), vel=orc.vel.copy(), prev_d=orc.prev_d.astype(F32),
                        flags=orc.flags.copy(), counters=orc.counters.copy()))
    return out


@pytest.mark.parametrize("n,world,commands", CASES)
def test_members_sit_on_their_thresholds_and_the_oracle_decides_as_tagged(oracle_mod, n, world, commands):
    b = tl.make_threshold_batch(n, world, commands)
    s1, s2 = _stepped(oracle_mod, b)
    lim = tl.limits(world)
    sides = {}
    for g in b["egos"]:
        e, i, cls = g["env"], g["agent"], g["cls"]
        ctx = tl.describe(b, e, i)
        r, dn, fl = float(s1["rew"][e, i]), int(s1["done"][e, i]), int(s1["flags"][e, i])
        if cls in ("C", "Ct", "H", "CS", "GS"):
            j = g["other"]
            if cls == "GS":
                assert np.array_equal(s1["loc"][e, j], g["q_new"]), ctx                       # the model's coasting move
                seen = b["loc"][e, j] if i < j else s1["loc"][e, j]
            else:
                seen = s1["loc"][e, j]
            assert np.array_equal(s1["loc"][e, i], b["loc"][e, i]), ctx
            s = nl.squares(s1["loc"][e, i], seen)
            assert int(bits(s)) == int(bits(g["want"])), ctx                                  # obligation 1
            others = [k for k in range(n) if k not in (i, j)]
            if others and cls != "Ct":                                                       # nobody else decides anything
                assert nl.squares(s1["loc"][e, i], s1["loc"][e, others]).min() > lim["sq_sense"], ctx
            if cls == "H":
                assert bool(fl & COLLIDED) == g["expect"], ctx                                # obligation 2
                assert int(s1["counters"][e, 2]) == (2 if g["expect"] else 0), ctx            # ego and neighbour, once each
                assert int(s2["counters"][e, 2]) == int(s1["counters"][e, 2]), ctx            # MUW:208: not counted again
                assert (r == -2.0) == bool(g["want"] <= lim["sq_two_r"]), ctx
            else:
                assert (r == -2.0) == g["expect"], ctx
                assert bool(fl & COLLIDED) == bool(s <= lim["sq_hard"] and (cls != "CS" or g["expect"])), ctx
            assert dn == 0 and not fl & DONE, ctx
        elif cls == "G":
            assert int(bits(s1["prev_d"][e, i])) == int(bits(g["want"])), ctx
            assert dn == int(g["expect"]) and bool(fl & DONE) == g["expect"], ctx
            assert (r == -2.0) == g["blocked"], ctx
            if g["expect"]:
                assert np.array_equal(s1["vel"][e, i], [0.0, 0.0]) and r > 9.0, ctx            # AG:41-42: NaN -> 0
            assert int(s1["counters"][e, 1]) == int(g["expect"]), ctx
        elif cls == "S":
            v = np.asarray(g["want"], np.float64)
            sq = tl.speed_sq(*v)
            fin = v / math.sqrt(sq) * 0.001 if g["expect"] else v                             # AG:40 on the model's velocity
            assert s1["vel"][e, i].tobytes() == fin.tobytes(), ctx
            assert float(s1["prev_d"][e, i]) < 0.45, ctx                                       # inside 0.5 m either way
            assert dn == int(g["expect"]) and bool(fl & DONE) == g["expect"], ctx
            assert int(s1["counters"][e, 1]) == int(g["expect"]), ctx
            off = {"2c/lim-1": -1, "2c/lim": 0, "2c/lim+1": 1}.get(g["member"])
            if off is not None:
                assert sq == float(nxt(tl.SPEED_SQ_LIM, off)), ctx
        elif cls == "O":
            ax = g["axis"]
            assert int(bits(s1["loc"][e, i, ax])) == int(bits(g["want"])), ctx
            edge = (lim["hi"] if "-hi/" in g["member"] else lim["lo"])[ax]
            assert int(bits(g["want"])) - int(bits(edge)) == (1 if g["expect"] else 0), ctx   # at the limit / one step outside
            assert dn == int(g["expect"]) and not fl & DONE, ctx
            assert ("coast" in g["member"]) == bool(b["vel"][e, i, ax] != 0), ctx
        if cls in IN_REWARD:
            sides.setdefault((cls, g["expect"]), []).append(r)
    for cls in IN_REWARD:                                                                     # obligation 3
        if (cls, True) in sides or (cls, False) in sides:
            yes, no = sides[(cls, True)], sides[(cls, False)]                                  # both sides occur
            gap = min(no) - max(yes) if cls in ("C", "Ct", "CS", "GS") else min(yes) - max(no)
            assert gap >= 0.5, (cls, gap)
    assert sorted((g["cls"], g["member"]) for g in b["egos"] if g["section"] == 0) == sorted(expected_members(n, world) * b["reps"])   # 6
    if n in tl.SECTIONED:
        for sec in (1, 2) if n != 4 else (1,):
            assert sorted((g["cls"], g["member"]) for g in b["egos"] if g["section"] == sec) == sorted(expected_members(n, world) * b["reps"])
    assert (b["loc"].shape[0] * n) % 64 != 0                                                   # a ragged last wavefront


@pytest.mark.parametrize("n,world,commands", [c for c in CASES if c[1] in ("r03", "r07")])
def test_box_members_do_not_end_the_episode_under_evaluate(oracle_mod, n, world, commands):
    b = tl.make_threshold_batch(n, world, commands)
    orc = tl.oracle_for(oracle_mod, b)
    _, _, d = orc.step(b["act"], evaluate=True)
    for g in b["egos"]:
        if g["cls"] == "O":
            assert d[g["env"], g["agent"]] == 0, tl.describe(b, g["env"], g["agent"])


@pytest.mark.parametrize("world,commands", [(w, c) for w in tl.WORLDS for c in ("f64", "f32")])
def test_n4_threshold_egos_on_the_fast_path_and_in_the_fallback(world, commands):
    b = tl.make_threshold_batch(4, world, commands)
    fb = nl.wave_fallback(b["loc"], tl.limits(world)["sq_sense"])
    per_cls = {}
    for g in b["egos"]:
        per_cls.setdefault(g["cls"], set()).add(bool(fb[g["env"] // 16]))
    if "Ct" in per_cls:   # these egos are near ties themselves: they pull their own wavefront into the fallback
        assert all(nl.lane_near_tie(b["loc"][g["env"]], g["agent"], tl.limits(world)["sq_sense"])
                   for g in b["egos"] if g["cls"] == "Ct")
        assert per_cls.pop("Ct") == {True}
    assert all(v == {True, False} for v in per_cls.values()), per_cls
    quiet = [g for g in b["egos"] if g["section"] == 0 and g["cls"] != "Ct"]
    assert not any(nl.env_near_tie(b["loc"][g["env"]], tl.limits(world)["sq_sense"]) for g in quiet)


@pytest.mark.parametrize("n,world,commands", [(n, w, c) for n in (7, 8, 13, 24) for w in tl.WORLDS for c in ("f64", "f32")])
def test_key_scan_threshold_egos_in_wavefronts_of_all_three_exits(n, world, commands):
    b = tl.make_threshold_batch(n, world, commands)
    cnt = tl.ego_tied_lane_counts(b)
    per_cls = {}
    for g, c in zip(b["egos"], cnt):
        per_cls.setdefault(g["cls"], set()).add("0" if c == 0 else ("1-6" if c <= 6 else ">=7"))
    ct = per_cls.pop("Ct", None)
    assert all(v == {"0", "1-6", ">=7"} for v in per_cls.values()), per_cls
    if ct is not None:    # a Ct ego is a tied lane itself: its own wavefront has at least that one
        assert ct == {"1-6", ">=7"}, ct
    if n in (7, 24):      # launch-shape independence: the egos change wavefront, and kind of wavefront, with the shape
        lanes = [tuple(tl.ego_lanes(b, W)) for W in (1, 2, 3, 4)]
        assert len(set(lanes)) >= 3
        assert len({tuple(tl.ego_tied_lane_counts(b, W).tolist()) for W in (1, 2, 3, 4)}) >= 3


# ---------------------------------------------------------------------------------------------------------------------------
# scripted bodies and levels; float64 positions
@pytest.mark.parametrize("L,B,leveled", [(4, 4, True), (8, 16, True), (4, 4, False), (8, 16, False)])
def test_body_and_level_members_sit_on_their_own_levels_thresholds(oracle_mod, L, B, leveled):
    """The neighbour of every C / CS / H ego is a body held still; each env's members stand at ITS level's limits; of every C / CS
    and O pair around a limit one member would be answered the other way round by the other level's limits; envs of the two
    levels alternate, so every wavefront holds both."""
    b = tl.make_ext_batch(L, B, leveled)
    E = b["loc"].shape[0]
    orc = tl.ext_setup(oracle_mod.OracleMulti(num_envs=E, nthreads=8, **tl.ext_kwargs(b)), b)
    assert np.array_equal(orc.level, b["level"]) and (E * L) % 64 != 0
    if leveled:
        assert np.array_equal(b["level"], np.arange(E) % 2) and b["epw"] >= 2
    _, rew, done = orc.step(b["act"])
    c1, p1 = orc.counters.copy(), orc.prev_d.copy()
    orc.step(b["act"])
    assert np.array_equal(orc.body, tl.body_records(b))                                        # the bodies stood still
    seen, flipped = set(), set()
    for g in b["egos"]:
        e, i, cls = g["env"], g["agent"], g["cls"]
        lim = tl.limits(tl.LEVELS[g["level"]])
        ctx = (e, i, cls, g["member"], g["level"])
        r, dn, fl = float(rew[e, i]), int(done[e, i]), int(orc.flags[e, i])
        if cls in ("C", "CS", "H"):
            assert g["other"] >= L
            s = nl.squares(orc.loc[e, i].astype(F32), b["loc"][e, g["other"]])
            assert int(bits(s)) == int(bits(g["want"])), ctx
            if cls == "H":
                assert bool(fl & COLLIDED) == g["expect"] and int(c1[e, 2]) == int(orc.counters[e, 2]) == int(g["expect"]), ctx
            else:
                assert (r == -2.0) == g["expect"], ctx
        elif cls == "G":
            assert int(bits(F32(p1[e, i]))) == int(bits(g["want"])), ctx
            assert dn == int(g["expect"]) and bool(fl & DONE) == g["expect"] and (r == -2.0) == g["blocked"], ctx
        else:
            assert int(bits(F32(orc.loc[e, i, g["axis"]]))) == int(bits(g["want"])) and dn == int(g["expect"]), ctx
        seen.add((g["level"], cls, g["member"]))
        if leveled and tl.other_level_disagrees(g):
            flipped.add((g["level"], cls))
    for lv, classes in enumerate(tl.LEVEL_CLASSES if leveled else tl.LEVEL_CLASSES[:1]):
        want = [(c, m) for c, m in expected_members(L + B, "r03") + expected_members(L + B, "cs")
                if c in classes and not m.endswith("coast")]
        assert sorted((c, m) for l, c, m in seen if l == lv) == sorted(set(want)), lv
    if leveled:
        assert flipped == {(0, "C"), (1, "CS"), (0, "O"), (1, "O")}


def test_float64_position_members_sit_one_float64_step_apart(oracle_mod):
    b = tl.make_threshold_batch64()
    orc = tl.oracle_for64(oracle_mod, b)
    _, rew, done = orc.step(b["act"])
    c1 = orc.counters.copy()
    orc.step(b["act"])
    sides, seen = {}, []
    w = tl.WORLD64
    for g in b["egos"]:
        e, i, cls = g["env"], g["agent"], g["cls"]
        ctx = (e, i, cls, g["member"])
        r, dn = float(rew[e, i]), int(done[e, i])
        step = {"prev": -1, "at": 0, "next": 1}
        if cls in ("C64", "H64"):
            lim = 2 * w["collider_radius"] if cls == "C64" else 1.0
            assert g["want"] == float(nxt(lim, step[g["member"].split("/")[0]])), ctx
            d = nl.nrm64(*(b["loc"][e, g["other"]] - b["loc"][e, i]))
            assert d == g["want"] == nl.nrm64(*(b["loc"][e, i] - b["loc"][e, g["other"]])), ctx
            if cls == "C64":
                assert (r == -2.0) == g["expect"], ctx
            else:
                assert int(c1[e, 2]) == int(orc.counters[e, 2]) == (2 if g["expect"] else 0), ctx
        elif cls == "G64":
            assert g["want"] == float(nxt(0.5, step[g["member"].split("/")[1]])), ctx
            assert nl.nrm64(*(b["tgt"][e, i] - b["loc"][e, i])) == g["want"] and dn == int(g["expect"]), ctx
        elif cls == "S64":
            assert dn == int(g["expect"]), ctx
        else:
            half = (w["x_size"], w["y_size"])[g["axis"]] / 2.0
            assert abs(g["want"]) in (half, float(nxt(half, 1))) and (abs(g["want"]) > half) == g["expect"], ctx
            assert dn == int(g["expect"]), ctx
        if cls in ("C64", "G64", "S64"):
            sides.setdefault((cls, g["expect"]), []).append(r)
        seen.append((cls, g["member"]))
    assert min(sides[("C64", False)]) - max(sides[("C64", True)]) >= 0.5
    for cls in ("G64", "S64"):
        assert min(sides[(cls, True)]) - max(sides[(cls, False)]) >= 0.5
    want = [(c, f"{m}/{o}") for c in ("C64", "H64") for m in ("prev", "at", "next") for o in ("below", "above")]
    want += [("G64", f"{k}/{m}") for k in ("axis", "diag") for m in ("prev", "at", "next")]
    want += [("S64", m) for c, m in expected_members(1, "r03") if c == "S"]
    want += [("O64", m) for c, m in expected_members(1, "r03") if c == "O"]
    assert sorted(seen) == sorted(want)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's own verdict
THR_GROUPS = thr_groups()[1]


def _group(key):
    data, meta = load_fixture("live_thresholds")
    assert meta["groups"] == [g[0] for g in THR_GROUPS]
    return {k.split("__", 1)[1]: v for k, v in data.items() if k.startswith(key + "__")}


@pytest.mark.parametrize("key,args", [(k, a) for k, kind, a in THR_GROUPS if kind == "muw"])
def test_oracle_equals_the_reference_at_the_thresholds(oracle_mod, key, args):
    """Every class member of C, Ct, H, CS, GS, G, S, O (and the clips) at 2 and 3 agents, all four worlds, float64 and float32
    commands: the oracle on the state the reference was given reproduces the record bit for bit, the reward included."""
    n, world, cmd = args
    ref = _group(key)
    b = tl.make_threshold_batch(n, world, cmd)
    envs = np.flatnonzero((b["section"] == 0) & ~b["filler"])
    np.testing.assert_array_equal(ref["env"], envs)
    for k in ("loc", "vel", "tgt", "init_d", "prev_d", "act"):                    # the record is of THESE states
        assert ref["in_" + k].tobytes() == b[k][envs].tobytes(), k
    assert sorted((g["cls"], g["member"]) for g in b["egos"] if g["env"] in set(envs.tolist())) \
        == sorted(expected_members(n, world) * b["reps"])
    sub = {k: b[k][envs] for k in ("loc", "vel", "tgt", "init_d", "prev_d", "act")}
    sub["world"] = world
    for ev in (False, True):
        orc = tl.oracle_for(oracle_mod, sub)
        for t in range(1 if ev else 2):
            _, rew, done = orc.step(sub["act"], evaluate=ev)
            tag = "eval" if ev else f"step{t + 1}"
            got = dict(rew=rew, done=done, loc=orc.loc, vel=orc.vel, prev_d=orc.prev_d, flags=orc.flags, counters=orc.counters[:, :3])
            for k, v in got.items():
                r = ref[f"{tag}_{k}"]
                bad = np.flatnonzero((np.asarray(v, np.float64) != np.asarray(r, np.float64)).reshape(len(envs), -1).any(1))
                assert bad.size == 0, (key, tag, k, [tl.describe(b, int(envs[x])) for x in bad[:4]])
                if k == "vel":
                    assert np.array_equal(np.signbit(v), np.signbit(r)), (key, tag, k)
    flips = {}
    for x, e in enumerate(envs):                                                   # and the reference decides as the tags say
        for g in b["egos"]:
            if g["env"] == e and g["cls"] in ("C", "Ct", "CS", "GS"):
                flips[g["member"]] = bool(ref["step1_rew"][x, g["agent"]] == -2.0)
                assert flips[g["member"]] == g["expect"], tl.describe(b, int(e))
            if g["env"] == e and g["cls"] in ("G", "S", "O"):
                assert int(ref["step1_done"][x, g["agent"]]) == int(g["expect"]), tl.describe(b, int(e))
                assert int(ref["eval_done"][x, g["agent"]]) == int(g["expect"] and g["cls"] != "O"), tl.describe(b, int(e))
            if g["env"] == e and g["cls"] == "H":
                assert int(ref["step1_counters"][x, 2]) == int(ref["step2_counters"][x, 2]) == (2 if g["expect"] else 0)


@pytest.mark.parametrize("key,args", [(k, a) for k, kind, a in THR_GROUPS if kind == "uw"])
def test_single_uav_oracle_equals_the_reference_at_the_thresholds(oracle_mod, key, args):
    box, cmd, fresh = args
    ref = _group(key)
    b = tl.make_uw_batch(box, cmd, fresh)
    for k in ("loc", "vel", "tgt", "init_d", "prev_d", "act"):
        assert ref["in_" + k].tobytes() == b[k].tobytes(), k
    orc = tl.uw_oracle_for(oracle_mod, b)
    act = b["act32"] if cmd == "f32" else b["act"]
    for t in (1, 2):
        obs, rew, done, info = orc.step(act)
        for k, v in dict(done=done, rew=rew, distance=info, obs=obs, loc=orc.loc, vel=orc.vel).items():
            r = ref[f"step{t}_{k}"]
            bad = np.flatnonzero((np.asarray(v, np.float64) != np.asarray(r, np.float64)).reshape(len(done), -1).any(1))
            assert bad.size == 0, (key, t, k, [(b["egos"][x]["cls"], b["egos"][x]["member"]) for x in bad[:4]])
    for g in b["egos"]:
        assert int(ref["step1_done"][g["env"]]) == int(g["expect"]), (key, g["member"])
        if g["cls"] == "G":
            assert int(bits(F32(ref["step1_distance"][g["env"]]))) == int(bits(g["want"]))
            assert (ref["step1_rew"][g["env"]] > 900) == g["expect"]
        else:
            assert int(bits(F32(ref["step1_loc"][g["env"], g["axis"]]))) == int(bits(g["want"]))

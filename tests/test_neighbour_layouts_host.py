"""The crafted neighbour layouts of tests/neighbour_layouts.py (CPU): deterministic, every class present at every agent count
where it can exist, both kinds of wavefront present at N = 4, and the host model of the float32 neighbour arithmetic agreeing
with the oracle's observe() on the crafted batches.  This is what guarantees that tests/test_gpu_neighbour_edges.py reaches
both scans of the 4-UAV one-step kernel and every tie / boundary case of the 2-5 UAV kernels."""
import math

import numpy as np
import pytest

import neighbour_layouts as nl

CASES = [(n, d) for n in (2, 3, 4, 5) for d in (9.0, 15.0, 7.3)]


def test_sq_limit_is_the_float32_sensing_boundary():
    for d in (9.0, 15.0, 7.3, 10.0, 0.5):
        sq = nl.sq_limit_lt(d)
        assert np.sqrt(sq) >= np.float32(d) and np.sqrt(np.nextafter(sq, np.float32(0))) < np.float32(d)


def test_generator_is_deterministic():
    for n, d in ((3, 9.0), (4, 7.3)):
        a, b = nl.make_batch(n, d, seed=0), nl.make_batch(n, d, seed=0)
        assert np.array_equal(a["loc"], b["loc"]) and np.array_equal(a["vel"], b["vel"])
        assert np.array_equal(a["cls"], b["cls"]) and np.array_equal(a["ego"], b["ego"])
        a64, b64 = nl.make_batch64(n, d), nl.make_batch64(n, d)
        assert np.array_equal(a64["loc"], b64["loc"])
    assert not np.array_equal(nl.make_batch(4, 9.0, seed=1)["loc"], nl.make_batch(4, 9.0, seed=0)["loc"])


@pytest.mark.parametrize("n,d_sense", CASES)
def test_every_class_is_present(n, d_sense):
    b = nl.make_batch(n, d_sense)
    sq = b["sq_sense"]
    seen = set()
    for e in range(len(b["cls"])):
        tags = nl.classify(b["loc"][e], int(b["ego"][e]), sq)
        assert b["cls"][e] in tags, (e, b["cls"][e], tags)
        seen |= tags
    assert set(nl.classes_possible(n)) <= seen
    if n in (4, 5):
        assert len(b["cls"]) % (64 // n) != 0   # a ragged last wavefront


@pytest.mark.parametrize("d_sense", [9.0, 15.0, 7.3])
def test_both_scan_paths_are_reached_at_n4(d_sense):
    b = nl.make_batch(4, d_sense)
    loc, sq, cls = b["loc"], b["sq_sense"], b["cls"]
    fb = nl.wave_fallback(loc, sq)
    wave = np.arange(len(cls)) // 16
    assert len(fb) == len(b["kinds"]) and list(fb) == [k == "fallback" for k in b["kinds"]]
    assert fb.any() and (~fb).any() and len(cls) % 16 != 0
    # fast wavefronts of A / B / E / G lanes only exist, and B lanes sit in some of them
    pure = [w for w in range(len(fb)) if not fb[w] and set(cls[wave == w]) <= {"A", "B", "E", "G0", "G1"}]
    assert pure and any("B" in cls[wave == w] for w in pure)
    # a single C or D env is what pulls a wavefront into the exact scan
    for w in np.flatnonzero(fb):
        envs = np.flatnonzero(wave == w)
        tied = [e for e in envs if nl.env_near_tie(loc[e], sq)]
        if len(envs) == 16:
            assert len(tied) == 1 and cls[tied[0]] in nl.FALLBACK_CLASSES
    for c in ("C", "D"):
        lanes = np.flatnonzero(cls == c)
        assert lanes.size >= 2 and fb[wave[lanes]].all()
        assert any(nl.lane_near_tie(loc[e], int(b["ego"][e]), sq) for e in lanes)


@pytest.mark.parametrize("n,d_sense", CASES)
def test_host_model_matches_oracle_observe(oracle_mod, n, d_sense):
    b = nl.make_batch(n, d_sense)
    E = len(b["cls"])
    orc = oracle_mod.OracleMulti(num_envs=E, num_agents=n, d_sense=d_sense, x_size=80.0, y_size=80.0)
    orc.reset_philox(1)
    orc.set_state(loc=b["loc"], vel=b["vel"])
    obs = orc.observe()
    ds = np.float32(d_sense)
    for e in range(E):
        for i in range(n):
            nb = nl.nearest_two(b["loc"][e], i, b["sq_sense"])
            theta = math.atan2(b["vel"][e, i, 1], b["vel"][e, i, 0])
            for k in range(2):
                if k < len(nb):
                    j, dj = nb[k]
                    assert obs[e, i, 4 + 3 * k] == float(np.float32(dj) / ds), (e, i, k)   # distance column exact
                    h = math.atan2(b["vel"][e, j, 1], b["vel"][e, j, 0]) - theta
                    want = math.atan2(math.sin(h), math.cos(h)) / math.pi
                    assert abs(obs[e, i, 6 + 3 * k] - want) < 1e-12, (e, i, k)                # identity via the heading
                else:
                    assert obs[e, i, 4 + 3 * k] == 1.0 and obs[e, i, 6 + 3 * k] == 0.0, (e, i, k)
    # headings are distinct: a wrong neighbour moves a heading column by at least ~2 / n - 0.1
    th = np.arctan2(b["vel"][..., 1], b["vel"][..., 0])
    for e in range(E):
        d = np.abs(th[e][:, None] - th[e][None])
        d = np.minimum(d, 2 * np.pi - d) / np.pi
        assert (d + np.eye(n) * 9).min() > 2.0 / n - 0.1


def test_zero_commands_keep_the_layout_for_step(oracle_mod):
    """The GPU test steps the crafted layouts with zero velocity and zero commands: positions stay where they were built."""
    b = nl.make_batch(4, 9.0)
    E = len(b["cls"])
    orc = oracle_mod.OracleMulti(num_envs=E, num_agents=4, d_sense=9.0, x_size=80.0, y_size=80.0)
    orc.reset_philox(1)
    orc.set_state(loc=b["loc"], vel=np.zeros_like(b["vel"]))
    orc.step(np.zeros((E, 4, 2), np.float32))
    assert np.array_equal(orc.loc.astype(np.float32), b["loc"])


@pytest.mark.parametrize("n,d_sense", [(3, 15.0), (4, 9.0), (5, 7.3)])
def test_float64_layouts_hit_ties_and_the_boundary(oracle_mod, n, d_sense):
    b = nl.make_batch64(n, d_sense)
    loc = b["loc"]
    E = len(b["cls"])
    hits = {"tie": 0, "below": 0, "at": 0, "above": 0, "tied_edge": 0}
    for e in range(E):
        i = int(b["ego"][e])
        d = sorted(nl.nrm64(*(loc[e, j] - loc[e, i])) for j in range(n) if j != i)
        if b["cls"][e] == "A64":
            hits["tie"] += d[0] == d[1]
        else:
            below, edge, above = np.nextafter(d_sense, 0.0), d_sense, np.nextafter(d_sense, np.inf)
            hits["below"] += d[0] == below
            hits["at"] += d[0] == edge
            hits["above"] += d[0] == above
            hits["tied_edge"] += d[0] == d[1] and d[0] in (below, edge, above)
    assert all(v > 0 for v in hits.values()), hits
    orc = oracle_mod.OracleMulti(num_envs=E, num_agents=n, d_sense=d_sense, x_size=80.0, y_size=80.0)
    orc.reset_philox(1)
    orc.set_state(loc=loc, vel=b["vel"])
    orc.f64pos[:] = 1
    obs = orc.observe()
    for e in range(E):   # in range iff d < d_sense in double
        i = int(b["ego"][e])
        nin = sum(nl.nrm64(*(loc[e, j] - loc[e, i])) < d_sense for j in range(n) if j != i)
        assert (obs[e, i, 4] < 1.0) == (nin >= 1) and (obs[e, i, 7] < 1.0) == (nin >= 2)

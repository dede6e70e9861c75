"""Host-side checks of prioritized replay (libuavx_prio.so, include/uavx_prio.h): the library builds for gfx950 without a
GPU and carries its source hash, exports exactly what its header declares, refuses every bad argument before touching a
device, its kernels use no scratch and spill nothing, the actor library it stands beside is untouched, and the numpy
restatement the GPU tests trust (prio_ref.py) follows the header's refresh rules entry by entry, draws entries with
frequencies p / total, and gives weights proportional to 1 / p at beta = 1."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import prio_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _xlib():
    from gym_uav_collision_avoidance_amd import _prio_lib
    _prio_lib.build()
    return _prio_lib


def _kernels():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr.kernel_table(_xlib().LIB_PATH)


# ---- the library ----------------------------------------------------------------------------------------------------------

def test_library_cross_compiles_and_carries_its_source_hash():
    x = _xlib()
    assert os.path.basename(x.LIB_PATH) == "libuavx_prio.so" and os.path.isfile(x.LIB_PATH)
    assert x.HEADER == os.path.join(ROOT, "include", "uavx_prio.h") and x.HEADER in x._sources()
    assert any(f.endswith(os.path.join("prio_csrc", "uavx_prio.hip")) for f in x._sources())
    blob = open(x.LIB_PATH, "rb").read()
    assert f"UAVX_PRIO_SRC_HASH={x.source_hash()}".encode() + b"\0" in blob and b"gfx950" in blob
    assert x._up_to_date()
    mk = open(os.path.join(x.CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, re.M).group(1)
    actor_mk = open(os.path.join(ROOT, "gym_uav_collision_avoidance_amd", "actor_csrc", "Makefile")).read()
    assert flags == re.search(r"^HIPFLAGS \?= (.*)$", actor_mk, re.M).group(1)
    assert "UAVX_PRIO_SRC_HASH" in mk and "OUT ?= libuavx_prio.so" in mk and "SRCHASH ?=" in mk
    assert "libuavx_prio.so.tmp*" in open(os.path.join(ROOT, ".gitignore")).read().split()


def test_library_exports_exactly_what_the_header_declares():
    x = _xlib()
    hdr = open(x.HEADER).read()
    declared = set(re.findall(r"\b(uavx_prio_[a-z_0-9]*)\s*\(", hdr))
    assert declared == set(x.SYMBOLS) == {"uavx_prio_version", "uavx_prio_state_bytes", "uavx_prio_refresh",
                                          "uavx_prio_sample", "uavx_prio_update"}
    assert x.SYMBOLS[0] == "uavx_prio_version"
    lib = x.load()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.uavx_prio_version() == x.ABI_VERSION == 1 and "#define UAVX_PRIO_VERSION 1" in hdr
    for name, value in (("ONE", x.ONE), ("MAX_ENTRIES", x.MAX_ENTRIES), ("MAX_ROWS", x.MAX_ROWS), ("MAX_TOWERS", x.MAX_TOWERS)):
        assert f"#define UAVX_PRIO_{name} {value}" in hdr, name
    assert x.ONE == 2 ** 16 == prio_ref.ONE and x.MAX_ENTRIES == 2 ** 26
    # the structs the binding fills have the header's fields, in its order
    for cname, cls in (("uavx_prio_record", x.Record), ("uavx_prio_state", x.State), ("uavx_prio_sample_args", x.SampleArgs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.search(r"(\w+)\s*$", d).group(1) for d in body.split(";") if d.strip()]
        assert fields == [n for n, _ in cls._fields_], cname
    assert ctypes.sizeof(x.Record) == x.RECORD_BYTES == 32


def test_the_actor_library_is_untouched():
    """The constraint this library exists for: libuavx_actor.so's units, sources and hash are pinned by other tests."""
    from gym_uav_collision_avoidance_amd import _actor_lib
    assert len(_actor_lib.UNITS) == 11 and _actor_lib.UNITS[-1].word == "weighted critic-gradient"
    assert not any("prio" in os.path.basename(f) for f in _actor_lib._sources())
    assert _actor_lib.source_hash() == "c6725b15f59f1983"
    # (a056e385b4f6651e before this library existed; moved twice since: when the weighted critic gradient became a unit, and from
    # 17c0e2c29cadcdb4 when its replay unit and this library took the ring's view from common_csrc/.  No file of prio_csrc/ is among
    # its sources, as before)
    pkg = os.path.join(ROOT, "gym_uav_collision_avoidance_amd")
    assert os.path.isdir(os.path.join(pkg, "prio_csrc")) and not os.path.exists(os.path.join(pkg, "replay_csrc"))


def test_state_bytes():
    x = _xlib()
    lib = x.load()
    n = ctypes.c_int64(-1)
    sizes = []
    for entries in (1, 63, 64, 65, 4096, 4097, 17920, 262144, 262145, 1052672, 2 ** 26):
        assert lib.uavx_prio_state_bytes(entries, ctypes.byref(n)) == x.OK
        n1 = -(-entries // 64)
        n2 = -(-n1 // 64)
        assert n.value % 16 == 0 and n.value >= 8 * (n1 + n2) + 8 * n2
        sizes.append(n.value)
    assert sizes == sorted(sizes) and sizes[-1] < 2 ** 24
    for entries in (0, -1, 2 ** 26 + 1, 2 ** 40):
        assert lib.uavx_prio_state_bytes(entries, ctypes.byref(n)) == x.ERR_INVALID_ARG
    assert lib.uavx_prio_state_bytes(4096, None) == x.ERR_INVALID_ARG


def test_bad_arguments_refused_before_any_device_call():
    x = _xlib()
    lib = x.load()
    P = 64                        # never dereferenced: every call below fails its argument check first
    bad = x.ERR_INVALID_ARG

    def ring(**kw):
        r = x.ReplayRing(obs=P, act=P, rew=P, done=P, skip=P, trunc=P, ended=P, slots=6, envs=8, agents=4, learners=4)
        for k, v in kw.items():
            setattr(r, k, v)
        return ctypes.pointer(r)

    def state(**kw):
        s = x.State(ring=ring(), count=3, count_dev=None, table=P, sums=P, sums_bytes=1 << 20, rec=P)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def args(**kw):
        a = x.SampleArgs(u=P, rows=256, stratified=1, beta=0.4, beta_dev=None, state=P, action=P, reward=P, next_state=P,
                         mask=P, truncated=P, ended=P, key=P, weight=P)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refresh(**kw):
        return lib.uavx_prio_refresh(ctypes.byref(state(**kw)), None)

    def sample(st=None, **kw):
        return lib.uavx_prio_sample(ctypes.byref(st or state()), ctypes.byref(args(**kw)), None)

    def update(st=None, key=P, q=P, towers=2, y=P, y_stride=1, rows=256, alpha=0.6, eps=1e-6):
        return lib.uavx_prio_update(ctypes.byref(st or state()), key, q, towers, y, y_stride, rows, alpha, eps, None)

    need = ctypes.c_int64()
    assert lib.uavx_prio_state_bytes(6 * 8 * 4, ctypes.byref(need)) == x.OK
    # the shared state, through all three entries
    states = [dict(ring=ctypes.POINTER(x.ReplayRing)())]
    states += [dict(ring=ring(**{name: None})) for name in ("obs", "act", "rew", "done")]
    states += [dict(ring=ring(**{n: None for n in miss})) for miss in
               (("skip",), ("trunc",), ("ended",), ("skip", "trunc"), ("trunc", "ended"), ("skip", "ended"))]
    states += [dict(ring=ring(slots=s)) for s in (1, 0, -3, 2 ** 31)]
    states += [dict(ring=ring(envs=0)), dict(ring=ring(agents=0))]
    states += [dict(ring=ring(learners=n)) for n in (0, -1, 5)]
    states += [dict(ring=ring(obs=68)), dict(ring=ring(act=68)), dict(ring=ring(rew=66))]
    # over capacity: 2^26 + 1 slot's worth, and sizes whose product overflows 64 bits
    states += [dict(ring=ring(slots=2 ** 13 + 1, envs=2 ** 11, agents=4, learners=4)),
               dict(ring=ring(slots=2 ** 31 - 1, envs=2 ** 31 - 1, agents=2 ** 31 - 1, learners=2 ** 31 - 1))]
    states += [dict(count=0), dict(count=-1), dict(count=0, count_dev=P + 4)]
    states += [dict(table=None), dict(table=P + 2), dict(sums=None), dict(sums=P + 8), dict(rec=None), dict(rec=P + 4),
               dict(sums_bytes=need.value - 1), dict(sums_bytes=0)]
    for kw in states:
        assert refresh(**kw) == bad, kw
        assert sample(state(**kw)) == bad and sample(state(**kw), rows=0) == bad, kw
        assert update(state(**kw)) == bad and update(state(**kw), rows=0) == bad, kw
    assert lib.uavx_prio_refresh(None, None) == bad and lib.uavx_prio_sample(None, ctypes.byref(args()), None) == bad
    assert lib.uavx_prio_sample(ctypes.byref(state()), None, None) == bad
    assert lib.uavx_prio_update(None, P, P, 1, P, 1, 4, 0.6, 1e-6, None) == bad
    # the sample call
    for rows in (-1, 2 ** 20 + 1, 2 ** 40):
        assert sample(rows=rows) == bad, rows
    for s in (2, -1):
        assert sample(stratified=s) == bad
    for beta in (-0.01, 1.01, float("nan"), float("inf")):
        assert sample(beta=beta) == bad, beta
    assert sample(beta=7.0, beta_dev=P + 2) == bad
    for name in ("u", "state", "action", "reward", "next_state", "mask", "key", "weight"):
        assert sample(**{name: None}) == bad, name
    assert sample(truncated=None) == bad and sample(ended=None) == bad and sample(rows=0, truncated=None) == bad
    assert sample(state=68) == bad and sample(next_state=68) == bad and sample(action=68) == bad and sample(key=68) == bad
    # the update call
    for rows in (-1, 2 ** 20 + 1):
        assert update(rows=rows) == bad, rows
    for towers in (0, 3, -1):
        assert update(towers=towers) == bad, towers
    assert update(y=None, towers=2) == bad and update(y_stride=0) == bad and update(y_stride=-1) == bad
    for alpha in (-0.1, 1.1, float("nan")):
        assert update(alpha=alpha) == bad and update(alpha=alpha, rows=0) == bad, alpha
    for eps in (0.0, -1e-6, float("nan"), float("inf")):
        assert update(eps=eps) == bad and update(eps=eps, rows=0) == bad, eps
    assert update(key=None) == bad and update(q=None) == bad and update(key=P + 4) == bad and update(y=P + 2) == bad
    # rows = 0 enqueues nothing and looks at no buffer; the other arguments are still checked
    assert sample(rows=0, u=None, state=None, key=None, weight=None) == x.OK
    assert sample(rows=0, truncated=None, ended=None) == x.OK
    assert update(rows=0, key=None, q=None, y=None, towers=1) == x.OK


def test_kernels_use_no_scratch_and_spill_nothing():
    rows = [r for r in _kernels() if r["name"].startswith("uavx_prio_k::")]
    assert sorted(r["name"].split("::")[1] for r in rows) == ["refresh_leaves", "refresh_top", "sample_rows", "update_clear",
                                                              "update_max"]
    assert len(rows) == len(_kernels())                           # every kernel of the library is in the namespace
    # kernel -> (LDS bytes, VGPRs) as DESIGN.md §23 documents them: refresh_leaves keeps per-wavefront partials (64 B) and
    # the loads of 16 nodes in registers; refresh_top 256 level-3 sums, 64 level-4 slots and its partials (2 752 B)
    documented = {"refresh_leaves": (64, 82), "refresh_top": (2752, 29), "sample_rows": (0, 37), "update_clear": (0, 15),
                  "update_max": (0, 30)}
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for r in rows:
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["private_segment_fixed_size"] == 0, r
        lds, vgprs = documented[r["name"].split("::")[1]]
        assert r["group_segment_fixed_size"] == lds, r
        assert r["agpr_count"] == 0 and r["vgpr_count"] <= vgprs, r
        assert f"| `{r['name'].split('::')[1]}` | {lds} | {vgprs} |" in design, r["name"]


# ---- the restatement -------------------------------------------------------------------------------------------------------

L_, E_, N_, NL_ = 6, 4, 3, 2


def _flags(seed, packed, rate=0.3):
    g = np.random.default_rng(seed)
    done = (g.random((L_, E_, N_)) < 0.3).astype(np.uint8)
    skip = (g.random((L_, E_)) < rate).astype(np.uint8)
    if packed:
        done[:, :, 0] |= skip * 2 + (g.random((L_, E_)) < 0.5).astype(np.uint8) * 8
        return done, None
    return done, skip


def _refresh_by_entry(table, rec, count, done, skip):
    """The header's refresh rules one entry at a time, in Python scalars."""
    c = max(1, count)
    T = L_ - 1
    lo = max(0, c - T)
    out = table.copy()
    for s in range(L_):
        ks = [k for k in range(lo, c) if k % L_ == s]
        assert len(ks) <= 1
        for e in range(E_):
            skipped = bool(done[s, e, 0] & 2) if skip is None else bool(skip[s, e])
            for i in range(NL_):
                if not ks or skipped:
                    out[s, e, i] = 0
                elif ks[0] >= max(rec.seen, lo):
                    out[s, e, i] = rec.p_max
    pos = [int(v) for v in out.ravel() if v > 0]
    return out, prio_ref.Record(total=sum(pos), p_min=min(pos) if pos else 0, p_max=rec.p_max, seen=c, valid=len(pos))


@pytest.mark.parametrize("packed", [False, True])
def test_refresh_restatement_equals_a_per_entry_loop(packed):
    g = np.random.default_rng(11 + packed)
    done, skip = _flags(3 + packed, packed)
    for counts in ((1, 2, 3), (3, 5, 6), (4, 5, 9, 14), (0, 1), (7, 7, 20)):        # below, at and past the wrap
        table, rec = np.zeros((L_, E_, NL_), dtype=np.uint32), prio_ref.new_record()
        want_t, want_r = table.copy(), rec
        for n, count in enumerate(counts):
            table, rec = prio_ref.refresh(table, rec, count, done, skip)
            want_t, want_r = _refresh_by_entry(want_t, want_r, count, done, skip)
            assert np.array_equal(table, want_t) and rec == want_r, (counts, count)
            assert table[max(1, count) % L_].sum() == 0                             # the head slot is never drawn
            assert rec.seen == max(1, count) and rec.valid == int((table > 0).sum())
            # priorities move between refreshes, as an update would move them
            hit = g.random(table.shape) < 0.5
            table = np.where(hit & (table > 0), g.integers(1, 2 ** 32, table.shape, dtype=np.uint64), table).astype(np.uint32)
            want_t = table.copy()
            rec = want_r = rec._replace(p_max=max(rec.p_max, int(table.max())))
    # every env a skip row: nothing can be drawn
    done0 = np.zeros((L_, E_, N_), dtype=np.uint8)
    table, rec = prio_ref.refresh(np.zeros((L_, E_, NL_), dtype=np.uint32), prio_ref.new_record(), 9, done0,
                                  np.ones((L_, E_), dtype=np.uint8))
    assert rec.total == 0 and rec.p_min == 0 and rec.valid == 0 and not table.any()


def test_draw_frequencies_converge_to_p_over_total():
    """200 000 draws over a 12-entry table: every entry within 5 sigma of its binomial expectation."""
    g = np.random.default_rng(5)
    L, E, NL = 3, 2, 2
    table = np.array([3000, 65536, 3 * 65536, 0, 2 ** 18, 20000, 65536, 0, 0, 0, 0, 0], dtype=np.uint32).reshape(L, E, NL)
    assert not table[2].any()                                      # count = 2: slot 2 is the head
    done = np.zeros((L, E, 3), dtype=np.uint8)
    skip = np.zeros((L, E), dtype=np.uint8)
    rec = prio_ref.Record(total=int(table.sum(dtype=np.uint64)), p_min=3000, p_max=2 ** 18, seen=2, valid=int((table > 0).sum()))
    obs = g.standard_normal((L, E, 3, 10)).astype(np.float32)
    act, rew = obs[..., :2].copy(), obs[..., 0].copy()
    B = 200_000
    for stratified in (False, True):
        u = g.random(B, dtype=np.float32)
        got = prio_ref.sample(u, table, rec, 2, obs, act, rew, done, skip, skip, skip, stratified=stratified, beta=1.0)
        freq = np.bincount(got.flat, minlength=table.size)
        p = table.reshape(-1).astype(np.float64) / rec.total
        sigma = np.sqrt(B * p * (1 - p))
        assert np.all(np.abs(freq - B * p) <= 5 * sigma + 1e-9), (stratified, freq, B * p)
        assert freq[table.reshape(-1) == 0].sum() == 0
        # beta = 1: weight · p is the constant p_min
        w = got.weight.astype(np.float64) * table.reshape(-1)[got.flat]
        assert np.allclose(w, rec.p_min, rtol=2e-7, atol=0)
        assert got.weight.max() == np.float32(1.0)                 # at the entry of priority p_min
        # the key names the step, the env and the agent
        s, rest = got.flat // (E * NL), got.flat % (E * NL)
        assert np.array_equal(got.key, s * (E * NL) + rest)        # count = 2 <= T: step k lies in slot k
        assert np.array_equal(got.state, obs[s, rest // NL, rest % NL])


def test_priority_of_a_td_error():
    p = prio_ref.priority(np.array([0.0, 1.0, 0.5, np.nan, np.inf, 1e9, 65535.99], dtype=np.float32), 1.0, 1e-6)
    assert p.tolist() == [1, 65536, 32768, 1, 2 ** 32 - 1, 2 ** 32 - 1, int(np.floor((np.float64(np.float32(65535.99)) + 1e-6) * 65536 + 0.5))]
    # alpha = 0 makes every finite error 1.0; a NaN still gives 1 and +inf the top: they are settled before the exponent
    assert prio_ref.priority(np.array([0.0, 3.0, np.inf, np.nan], dtype=np.float32), 0.0, 1e-6).tolist() == [
        65536, 65536, 2 ** 32 - 1, 1]
    assert prio_ref.priority(np.array([np.inf, np.nan], dtype=np.float32), 0.6, 1e-6).tolist() == [2 ** 32 - 1, 1]
    assert prio_ref.priority(np.array([4.0], dtype=np.float32), 0.5, 1e-6).tolist() == [131072]
    d = prio_ref.delta_of(np.array([[1.0, 5.0, np.nan, 2.0], [3.0, 1.0, 1.0, np.nan]], dtype=np.float32),
                          np.array([2.0, 2.0, 2.0, 2.0], dtype=np.float32))
    assert d[:2].tolist() == [1.0, 3.0] and np.isnan(d[2:]).all()
    # duplicates end at the maximum; stale and negative keys are ignored
    table = np.full((L_, E_, NL_), 9, dtype=np.uint32)
    rec = prio_ref.new_record()._replace(seen=8)
    per = E_ * NL_
    key = np.array([7 * per + 3, 7 * per + 3, 7 * per + 3, -1, 2 * per, 8 * per + 1, 3 * per + 5], dtype=np.int64)
    q = np.array([0.25, 2.0, 1.0, 9.0, 9.0, 9.0, 0.5], dtype=np.float32)
    out, rec2 = prio_ref.update(table, rec, 8, key, q, None, alpha=1.0, eps=1e-6)     # window: steps 3..7
    want = table.copy()
    want[7 % L_].reshape(-1)[3] = 131072
    want[3 % L_].reshape(-1)[5] = 32768
    assert np.array_equal(out, want) and rec2.p_max == 131072 and rec2.seen == 8


# ---- what the Python layer refuses on the host -----------------------------------------------------------------------------

def test_sampler_and_learner_keywords_refused_on_the_host():
    from gym_uav_collision_avoidance_amd.learners import FusedDDPG, FusedSAC, FusedTD3
    from gym_uav_collision_avoidance_amd.prioritized_replay import PrioritizedReplaySampler, check_prioritized
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    for other in (object(), None, {"obs": 1}, torch.zeros(3)):
        with pytest.raises(TypeError, match="uavx: PrioritizedReplaySampler takes a DeviceReplay"):
            PrioritizedReplaySampler(other)
    mem = DeviceReplay.__new__(DeviceReplay)                   # a ring on the CPU: there is no CPU path
    mem.obs = torch.zeros((L_, E_, N_, 10))
    with pytest.raises(ValueError, match="uavx: .*no CPU path"):
        PrioritizedReplaySampler(mem, alpha=7)                 # the ring's place is looked at first
    assert check_prioritized(0.6, 1e-6) == (0.6, 1e-6) and check_prioritized(0, 1) == (0.0, 1.0)
    for alpha in (-0.1, 1.5, float("nan"), "x", None):
        with pytest.raises(ValueError, match=r"alpha in \[0, 1\]"):
            check_prioritized(alpha, 1e-6)
    for eps in (0.0, -1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="finite eps > 0"):
            check_prioritized(0.6, eps)
    for rows in (-1, 2 ** 20 + 1):
        with pytest.raises(ValueError, match="uavx: PrioritizedReplaySampler takes 0..1048576 rows"):
            PrioritizedReplaySampler._rows(rows)
    # the learners check their keywords before they look for a device
    for cls in (FusedSAC, FusedTD3, FusedDDPG):
        with pytest.raises(ValueError, match=rf"uavx: {cls.__name__} takes a priority exponent alpha in \[0, 1\], got 1.5"):
            cls(device="cpu", prioritized=1.5)
        with pytest.raises(ValueError, match=rf"uavx: {cls.__name__} takes a finite eps > 0"):
            cls(device="cpu", prioritized=0.6, per_eps=0.0)
        with pytest.raises(ValueError, match="goes with n_step=1 and recency=0"):
            cls(device="cpu", prioritized=0.6, n_step=3)
        with pytest.raises(ValueError, match="goes with n_step=1 and recency=0"):
            cls(device="cpu", prioritized=0.6, recency=0.5)
        with pytest.raises(ValueError, match="uavx: the learners need a GPU"):
            cls(device="cpu", prioritized=0.6)

"""Host-side checks of the n-step replay sampler (libuavx_actor.so, include/uavx_nstep.h): the library builds for gfx950
without a GPU and carries its source hash, exports exactly what its header declares, refuses every bad argument before
touching a device, its kernels use no scratch and spill nothing, it is one unit of eleven beside the one-step interface it
shares its kernels with, and the numpy restatement the GPU tests trust (nstep_ref.py) equals a per-row loop written from
the header's prose, equals replay_ref.sample for one step, and draws step indices with a cumulative distribution of exactly (m/span)^2."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import nstep_ref
import replay_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _xlib():
    from gym_uav_collision_avoidance_amd import _actor_lib
    _actor_lib.build()
    return _actor_lib


def _kernels():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr.kernel_table(_xlib().LIB_PATH)


# ---- the library ----------------------------------------------------------------------------------------------------------

def test_library_cross_compiles_and_carries_its_source_hash():
    x = _xlib()
    assert os.path.basename(x.LIB_PATH) == "libuavx_actor.so" and os.path.isfile(x.LIB_PATH)
    assert x.NSTEP_HEADER == os.path.join(ROOT, "include", "uavx_nstep.h") and x.NSTEP_HEADER in x._sources()
    assert any(f.endswith(os.path.join("actor_csrc", "uavx_replay.hip")) for f in x._sources())
    assert f"UAVX_ACTOR_SRC_HASH={x.source_hash()}".encode() + b"\0" in open(x.LIB_PATH, "rb").read()
    assert x._up_to_date()
    mk = open(os.path.join(x.CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, re.M).group(1).split()
    assert flags == "-O3 -std=c++17 --offload-arch=$(ARCH) -ffp-contract=off -fPIC -Wall -Wno-unused-function".split()
    assert "UAVX_ACTOR_SRC_HASH" in mk and "OUT ?= libuavx_actor.so" in mk and "SRCHASH ?=" in mk
    assert "uavx_nstep.h" in mk and "uavx_replay.hip" in mk
    # the kernels are gfx950 code objects
    assert b"gfx950" in open(x.LIB_PATH, "rb").read()


def test_library_exports_exactly_what_the_header_declares():
    x = _xlib()
    hdr = open(x.NSTEP_HEADER).read()
    declared = set(re.findall(r"\b(uavx_nstep_[a-z_0-9]*)\s*\(", hdr))
    assert declared == set(x.NSTEP_SYMBOLS) == {"uavx_nstep_version", "uavx_nstep_workspace_bytes", "uavx_nstep_sample"}
    unit, = [u for u in x.UNITS if u.word == "n-step replay"]
    assert x.NSTEP_SYMBOLS[0] == unit.version == "uavx_nstep_version" and tuple(unit.functions) == x.NSTEP_SYMBOLS
    lib = x.load()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.uavx_nstep_version() == x.NSTEP_ABI_VERSION == 1 and "#define UAVX_NSTEP_VERSION 1" in hdr
    assert f"#define UAVX_NSTEP_MAX {x.NSTEP_MAX}" in hdr and x.NSTEP_MAX == 8
    assert f"#define UAVX_NSTEP_MAX_ROWS {x.NSTEP_MAX_ROWS}" in hdr and x.NSTEP_MAX_ROWS == 2 ** 20
    assert f"#define UAVX_NSTEP_SINGLE_ROWS {x.NSTEP_SINGLE_ROWS}" in hdr and x.NSTEP_SINGLE_ROWS == 1024
    # the struct the binding fills has the header's fields, in its order
    body = re.search(r"typedef struct uavx_nstep_args \{(.*?)\} uavx_nstep_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", d).group(1) for d in body.split(";") if d.strip()]
    assert fields == [n for n, _ in x.NStepArgs._fields_]
    assert x.NStepArgs._fields_[0][1] is ctypes.POINTER(x.ReplayRing)


def test_one_library_serves_both_sampler_interfaces():
    x = _xlib()
    assert len(x.UNITS) == 11
    pkg = os.path.join(ROOT, "gym_uav_collision_avoidance_amd")
    assert not os.path.exists(os.path.join(pkg, "replay_csrc"))
    assert importlib.util.find_spec("gym_uav_collision_avoidance_amd._replayx_lib") is None
    assert [os.path.basename(f) for f in x._sources() if "nstep" in os.path.basename(f)] == ["uavx_nstep.h"]
    lib = x.load()                                            # one handle, one file: both interfaces resolve in it
    assert lib._name == x.LIB_PATH
    for name in x.NSTEP_SYMBOLS + x.REPLAY_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.uavx_nstep_version() == lib.uavx_replay_version() == 1


def test_workspace_bytes():
    x = _xlib()
    lib = x.load()
    n = ctypes.c_int64(-1)
    for rows in (0, 1, 1024):
        assert lib.uavx_nstep_workspace_bytes(rows, ctypes.byref(n)) == x.OK and n.value == 0
    sizes = []
    for rows in (1025, 2048, 2049, 2 ** 20):
        assert lib.uavx_nstep_workspace_bytes(rows, ctypes.byref(n)) == x.OK
        assert n.value >= 16 * rows + 8 * -(-rows // 1024) and n.value % 16 == 0
        sizes.append(n.value)
    assert sizes == sorted(sizes) and sizes[-1] < 2 ** 25
    for rows in (-1, 2 ** 20 + 1):
        assert lib.uavx_nstep_workspace_bytes(rows, ctypes.byref(n)) == x.ERR_INVALID_ARG
    assert lib.uavx_nstep_workspace_bytes(2048, None) == x.ERR_INVALID_ARG


def test_bad_arguments_refused_before_any_device_call():
    x = _xlib()
    lib = x.load()
    P = 64                        # never dereferenced: every call below fails its argument check first

    def ring(**kw):
        r = x.ReplayRing(obs=P, act=P, rew=P, done=P, skip=P, trunc=P, ended=P, slots=6, envs=8, agents=4, learners=4)
        for k, v in kw.items():
            setattr(r, k, v)
        return ctypes.pointer(r)

    def call(**kw):
        a = x.NStepArgs(ring=ring(), count=3, count_dev=None, u=P, u_cols=5, n_step=3, gamma=0.99, recency=0.5, rows=2048,
                        state=P, action=P, reward=P, next_state=P, mask=P, length=P, truncated=P, ended=P, workspace=P,
                        workspace_bytes=1 << 20)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.uavx_nstep_sample(ctypes.byref(a), None)

    bad = x.ERR_INVALID_ARG
    assert lib.uavx_nstep_sample(None, None) == bad                                           # NULL struct
    assert call(ring=ctypes.POINTER(x.ReplayRing)()) == bad                                   # NULL ring
    for name in ("obs", "act", "rew", "done"):
        assert call(ring=ring(**{name: None})) == bad, name
    for miss in (("skip",), ("trunc",), ("ended",), ("skip", "trunc"), ("trunc", "ended"), ("skip", "ended")):
        assert call(ring=ring(**{n: None for n in miss})) == bad, miss
    for slots in (1, 0, -3, 2 ** 31):
        assert call(ring=ring(slots=slots)) == bad, slots
    assert call(ring=ring(envs=0)) == bad and call(ring=ring(agents=0)) == bad
    for learners in (0, -1, 5):
        assert call(ring=ring(learners=learners)) == bad, learners
    assert call(ring=ring(obs=68)) == bad and call(ring=ring(act=68)) == bad                  # not 8-byte aligned
    for count in (0, -1):
        assert call(count=count) == bad, count
    assert call(count=0, count_dev=P + 4) == bad                                              # device count misaligned
    for rows in (-1, 2 ** 20 + 1, 2 ** 40):
        assert call(rows=rows) == bad, rows
    for n_step in (0, 9, -1):
        assert call(n_step=n_step) == bad, n_step
    for gamma in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        assert call(gamma=gamma) == bad, gamma
    for recency in (-0.01, 1.01, float("nan"), float("inf")):
        assert call(recency=recency) == bad, recency
    for u_cols in (4, 0, 2, 6, -5):
        assert call(u_cols=u_cols) == bad, u_cols
        assert call(u_cols=u_cols, recency=0.0) == bad, u_cols
    assert call(u_cols=3) == bad and call(u_cols=3, recency=1.0) == bad                       # three columns draw no coin
    for name in ("u", "state", "action", "reward", "next_state", "mask"):
        assert call(**{name: None}) == bad, name
        assert call(rows=256, **{name: None}) == bad, name
    assert call(truncated=None) == bad and call(ended=None) == bad                            # both or neither
    assert call(rows=0, truncated=None) == bad
    assert call(state=68) == bad and call(next_state=68) == bad and call(action=68) == bad
    need = ctypes.c_int64()
    assert lib.uavx_nstep_workspace_bytes(2048, ctypes.byref(need)) == x.OK
    assert call(workspace=None) == bad and call(workspace_bytes=need.value - 1) == bad and call(workspace_bytes=0) == bad
    assert call(workspace=P + 8) == bad                                                       # not 16-byte aligned
    # rows = 0 enqueues nothing and looks at no buffer; the other arguments are still checked
    assert call(rows=0, u=None, state=None, length=None, workspace=None, workspace_bytes=0) == x.OK
    assert call(rows=0, u_cols=3, recency=0.0, truncated=None, ended=None) == x.OK
    assert call(rows=0, n_step=9) == bad and call(rows=0, ring=ring(slots=1)) == bad and call(rows=0, gamma=0.0) == bad


def test_kernels_use_no_scratch_and_spill_nothing():
    rows = _kernels()
    rows = [r for r in rows if r["name"].startswith("uavx_replay_k::")]
    assert rows and not any("uavx_nstep_k::" in r["name"] for r in _kernels())
    names = sorted(r["name"] for r in rows)
    # one small and one gather kernel per n_step of 1..8 and flag layout, and the draw kernel
    assert sum("sample_small<" in n for n in names) == 16 and sum("sample_gather<" in n for n in names) == 16
    assert sum("sample_draw" in n for n in names) == 1 and len(names) == 33
    for r in rows:
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["private_segment_fixed_size"] == 0, r
        assert r["group_segment_fixed_size"] <= 8192, r
        # a workgroup of 1024 threads is 4 waves per SIMD: 512 / 4 registers each at the most
        assert r["agpr_count"] == 0 and r["vgpr_count"] <= 128, r


# ---- the restatement -------------------------------------------------------------------------------------------------------

L_, E_, N_, T_ = 6, 8, 4, 5


def _ring(seed, packed, skip_rate=0.2, done_rate=0.2, ended_rate=0.2):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn((L_, E_, N_, 10), generator=g)
    act = torch.rand((L_, E_, N_, 2), generator=g) * 2 - 1
    rew = torch.randn((L_, E_, N_), generator=g)
    done = (torch.rand((L_, E_, N_), generator=g) < done_rate).to(torch.uint8)
    skip = (torch.rand((L_, E_), generator=g) < skip_rate).to(torch.uint8)
    trunc = (torch.rand((L_, E_), generator=g) < 0.4).to(torch.uint8)
    ended = (torch.rand((L_, E_), generator=g) < ended_rate).to(torch.uint8)
    if packed:
        done[:, :, 0] |= skip * 2 + trunc * 8 + ended * 4
        return dict(obs=obs.numpy(), act=act.numpy(), rew=rew.numpy(), done=done.numpy(), skip=None, trunc=None, ended=None)
    return dict(obs=obs.numpy(), act=act.numpy(), rew=rew.numpy(), done=done.numpy(), skip=skip.numpy(), trunc=trunc.numpy(),
                ended=ended.numpy())


def _idx(u, n):
    """idx(u, n) of the header for one float32, in Python arithmetic on the float32 product."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = float(np.float32(u) * np.float32(n))
    if x != x or x < 0:
        return 0
    if x >= n:
        return n - 1
    return min(int(x), n - 1)


def _by_rows(u, ring, count, learners, n_step, gamma, recency):
    """The header's steps 1-4 one row at a time, in Python scalars: nothing shared with nstep_ref but the inputs."""
    obs, act, rew, done = ring["obs"], ring["act"], ring["rew"], ring["done"]

    def flag(name, bit, s, e):
        return bool(done[s, e, 0] & bit) if ring["skip"] is None else bool(ring[name][s, e])

    B = u.shape[2]
    c = max(count, 1)
    lo = max(0, c - T_)
    span = c - lo
    starts = []
    for j in range(B):
        draws = []
        for d in (0, 1):
            ka = _idx(u[d, 0, j], span)
            if u.shape[1] == 5 and u[d, 4, j] < np.float32(recency):
                ka = max(ka, _idx(u[d, 3, j], span))
            draws.append((lo + ka, _idx(u[d, 1, j], E_), _idx(u[d, 2, j], learners)))
        k, e, i = draws[1] if flag("skip", 2, draws[0][0] % L_, draws[0][1]) else draws[0]
        starts.append((k, e, i, not flag("skip", 2, k % L_, e)))
    out = []
    for j in range(B):
        before = [p for p in range(j + 1) if starts[p][3]]
        after = [p for p in range(j + 1, B) if starts[p][3]]
        src = before[-1] if before else (after[0] if after else B - 1)
        k, e, i, _ = starts[src]
        R, g, t = -0.0, 1.0, 0
        while True:
            s = (k + t) % L_
            R += g * float(rew[s, e, i])
            d = int(done[s, e, i] & 1)
            if (t == n_step - 1 or d or flag("ended", 4, s, e) or k + t + 1 >= c
                    or flag("skip", 2, (k + t + 1) % L_, e)):
                break
            g *= gamma
            t += 1
        length = t + 1
        out.append((obs[k % L_, e, i], act[k % L_, e, i], np.float32(R), obs[(k + length) % L_, e, i],
                    np.float32((1 - d) * g), flag("trunc", 8, s, e), flag("ended", 4, s, e), src, length))
    return out


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("n_step", [1, 2, 3, 8])
def test_restatement_equals_a_per_row_loop(n_step, packed):
    ring = _ring(7 * n_step + packed, packed)
    rng = np.random.default_rng(n_step)
    seen = 0
    for count in (1, 2, T_, T_ + 1, 14):
        for learners, recency, gamma in ((4, 0.0, 0.99), (3, 0.8, 0.9), (4, 1.0, 1.0)):
            for B in (1, 67):
                u = rng.random((2, 3 if recency == 0.0 and B == 1 else 5, B), dtype=np.float32)
                got = nstep_ref.sample(u, count=count, T=T_, num_learners=learners, n_step=n_step, gamma=gamma,
                                       recency=recency, **ring)
                want = _by_rows(u, ring, count, learners, n_step, gamma, recency)
                for j, w in enumerate(want):
                    g = (got.state[j], got.action[j], got.reward[j], got.next_state[j], got.mask[j], got.truncated[j],
                         got.ended[j], got.src[j], got.length[j])
                    for a, b in zip(g, w):
                        assert np.array_equal(a, b), (count, j, a, b)
                assert got.reward.dtype == np.float32 and got.mask.dtype == np.float32 and got.length.dtype == np.uint8
                assert (got.length >= 1).all() and (got.length <= n_step).all() and (got.reason > 0).all()
                seen |= int(np.bitwise_or.reduce(got.reason))
    # every one of the five conditions came up -- but a window of T_ steps meets its head before an 8th step
    assert seen == (31 if n_step <= T_ else 31 - nstep_ref.N_STEP) and sum(nstep_ref.REASONS.values()) == 31


@pytest.mark.parametrize("packed", [False, True])
def test_one_step_restatement_equals_replay_ref(packed):
    ring = _ring(40 + packed, packed, skip_rate=0.4)
    ring["rew"][:, ::2, 1] = -0.0                               # one step hands a reward of −0 on as it is
    rng = np.random.default_rng(5)
    for count in (1, 3, T_, T_ + 1, 14):
        for learners in (4, 3):
            for B in (1, 5, 300):
                u = rng.random((2, 3, B), dtype=np.float32)
                want = replay_ref.sample(u, count=count, T=T_, num_learners=learners, **ring)
                for gamma in (0.99, 1.0):
                    got = nstep_ref.sample(u, count=count, T=T_, num_learners=learners, n_step=1, gamma=gamma, **ring)
                    for x, w in zip(got[:8], want):
                        assert x.shape == w.shape and x.dtype == w.dtype and np.array_equal(x, w)
                    assert (got.length == 1).all() and np.array_equal(got.reward.view(np.int32), want[2].view(np.int32))
                    assert B < 300 or np.signbit(got.reward[got.reward == 0]).any()
                # five columns with recency 0 draw the same rows: columns 3 and 4 are not looked at
                u5 = np.concatenate([u, rng.random((2, 2, B), dtype=np.float32)], axis=1)
                got = nstep_ref.sample(u5, count=count, T=T_, num_learners=learners, n_step=1, gamma=0.99, **ring)
                assert all(np.array_equal(x, w) for x, w in zip(got[:8], want))


@pytest.mark.parametrize("span", [1, 2, 5, 7])
def test_recency_weighted_draw_has_a_square_law_exactly(span):
    """recency = 1 over the grid of all (u0, u3) = ((a + ½)/span, (b + ½)/span): k − lo = max(a, b), so the number of pairs
    with k − lo < m is exactly m² of span² -- the cumulative sum of weights proportional to m + ½ (0.25 + 0.5·m)."""
    count, T = 11, span                            # the count is past the horizon: the window holds T = span steps
    a, b = np.meshgrid(np.arange(span), np.arange(span), indexing="ij")
    B = span * span
    u = np.zeros((2, 5, B), dtype=np.float32)
    u[:, 0] = ((a.ravel() + 0.5) / span).astype(np.float32)
    u[:, 3] = ((b.ravel() + 0.5) / span).astype(np.float32)
    u[:, 4] = 0.5
    skip = np.zeros((T + 1, 3), dtype=bool)
    lo = count - T
    k, _, _, valid = nstep_ref.start_rows(u, count, T, 3, 2, skip, recency=1.0)
    assert valid.all() and np.array_equal(k - lo, np.maximum(a, b).ravel())
    for m in range(span + 1):
        assert int((k - lo < m).sum()) == m * m
    # the weights themselves: 2m + 1 pairs on index m, proportional to 0.25 + 0.5·m
    assert np.bincount(k - lo, minlength=span).tolist() == [2 * m + 1 for m in range(span)]
    # recency = 0, or a coin that is not below it, draws uniformly
    for recency, coin in ((0.0, 0.5), (0.5, 0.5), (0.5, np.nan), (1.0, 1.0)):
        u[:, 4] = coin
        k0 = nstep_ref.start_rows(u, count, T, 3, 2, skip, recency=recency)[0]
        assert np.bincount(k0 - lo, minlength=span).tolist() == [span] * span


# ---- what the Python layer refuses on the host -----------------------------------------------------------------------------

def test_sampler_and_learner_keywords_refused_on_the_host():
    from gym_uav_collision_avoidance_amd.fused_replay_nstep import NStepReplaySampler, check_n_step
    from gym_uav_collision_avoidance_amd.learners import FusedDDPG, FusedSAC, FusedTD3
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    for other in (object(), None, {"obs": 1}, torch.zeros(3)):
        with pytest.raises(TypeError, match="uavx: NStepReplaySampler takes a DeviceReplay"):
            NStepReplaySampler(other)
    mem = DeviceReplay.__new__(DeviceReplay)                   # a ring on the CPU: there is no CPU path
    mem.obs = torch.zeros((L_, E_, N_, 10))
    with pytest.raises(ValueError, match="uavx: .*no CPU path"):
        NStepReplaySampler(mem, n_step=99)                     # the ring's place is looked at first
    assert check_n_step(1, 0) == (1, 0.0) and check_n_step(8, 1) == (8, 1.0) and check_n_step(np.int64(3), 0.8) == (3, 0.8)
    for n in (0, 9, -1, 2.5, "3", None):
        with pytest.raises(ValueError, match=r"uavx: NStepReplaySampler takes n_step in 1\.\.8"):
            check_n_step(n, 0.0)
    for r in (-0.1, 1.5, float("nan"), "x", None):
        with pytest.raises(ValueError, match=r"uavx: NStepReplaySampler takes recency in \[0, 1\]"):
            check_n_step(3, r)
    for rows in (-1, 2 ** 20 + 1):
        with pytest.raises(ValueError, match="uavx: NStepReplaySampler takes 0..1048576 rows"):
            NStepReplaySampler._rows(rows)
    # the learners check their keywords before they look for a device
    for cls in (FusedSAC, FusedTD3, FusedDDPG):
        with pytest.raises(ValueError, match=rf"uavx: {cls.__name__} takes n_step in 1\.\.8, got 9"):
            cls(device="cpu", n_step=9)
        with pytest.raises(ValueError, match=rf"uavx: {cls.__name__} takes recency in \[0, 1\], got 1.5"):
            cls(device="cpu", recency=1.5)
        with pytest.raises(ValueError, match="uavx: the learners need a GPU"):
            cls(device="cpu", n_step=3, recency=0.8)

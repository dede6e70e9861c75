"""Host-side checks of the replay sampler in libuavx_actor.so (include/uavx_replay.h): the library builds for gfx950 without
a GPU with the new translation unit under the source hash, exports what its header declares, rejects bad arguments before
touching a device, its kernels stay within their resource budget, FusedReplaySampler refuses on the host what it cannot
run, and the numpy reference the GPU tests trust equals the torch expressions of DeviceReplay.sample on CPU tensors."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import replay_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _alib():
    from gym_uav_collision_avoidance_amd import _actor_lib
    _actor_lib.build()
    return _actor_lib


def _kernels():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr.kernel_table(_alib().LIB_PATH)


def test_replay_library_cross_compiles_and_hash_covers_header():
    a = _alib()
    assert a.REPLAY_HEADER in a._sources()
    assert any(f.endswith("uavx_replay.hip") for f in a._sources())
    assert f"UAVX_ACTOR_SRC_HASH={a.source_hash()}".encode() in open(a.LIB_PATH, "rb").read()
    mk = open(os.path.join(a.CSRC, "Makefile")).read()
    assert "uavx_replay.hip" in mk and "uavx_replay.h" in mk


def test_replay_exports_every_declared_symbol():
    a = _alib()
    hdr = open(a.REPLAY_HEADER).read()
    declared = set(re.findall(r"\b(uavx_replay_[a-z_0-9]*)\s*\(", hdr))
    assert declared == set(a.REPLAY_SYMBOLS), declared ^ set(a.REPLAY_SYMBOLS)
    assert set(a.REPLAY_SYMBOLS).isdisjoint(a.SYMBOLS + a.CRITIC_SYMBOLS + a.GRAD_SYMBOLS + a.OPTIM_SYMBOLS)
    lib = a.load()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.uavx_replay_version() == a.REPLAY_ABI_VERSION == 1
    assert f"#define UAVX_REPLAY_MAX_ROWS {a.REPLAY_MAX_ROWS}" in hdr and a.REPLAY_MAX_ROWS == 2 ** 20
    assert f"#define UAVX_REPLAY_SINGLE_ROWS {a.REPLAY_SINGLE_ROWS}" in hdr and a.REPLAY_SINGLE_ROWS == 1024
    from gym_uav_collision_avoidance_amd import fused_replay
    assert callable(fused_replay.FusedReplaySampler)


def test_replay_workspace_bytes():
    a = _alib()
    lib = a.load()
    n = ctypes.c_int64(-1)
    for rows in (0, 1, 1024):
        assert lib.uavx_replay_workspace_bytes(rows, ctypes.byref(n)) == a.OK and n.value == 0
    sizes = []
    for rows in (1025, 2048, 2049, 2 ** 20):
        assert lib.uavx_replay_workspace_bytes(rows, ctypes.byref(n)) == a.OK
        assert n.value >= 16 * rows + 8 * -(-rows // 1024) and n.value % 16 == 0
        sizes.append(n.value)
    assert sizes == sorted(sizes) and sizes[-1] < 2 ** 25
    for rows in (-1, 2 ** 20 + 1):
        assert lib.uavx_replay_workspace_bytes(rows, ctypes.byref(n)) == a.ERR_INVALID_ARG
    assert lib.uavx_replay_workspace_bytes(2048, None) == a.ERR_INVALID_ARG


def test_replay_bad_arguments_rejected_before_any_device_call():
    a = _alib()
    lib = a.load()
    P = 64                        # never dereferenced: every call below fails its argument check first

    def ring(**kw):
        r = a.ReplayRing(obs=P, act=P, rew=P, done=P, skip=P, trunc=P, ended=P, slots=6, envs=8, agents=4, learners=4)
        for k, v in kw.items():
            setattr(r, k, v)
        return ctypes.byref(r)

    def call(ring_=None, count=3, count_dev=None, u=P, rows=2048, s=P, a_=P, r=P, s2=P, m=P, tr=P, en=P, ws=P, ws_bytes=1 << 20):
        return lib.uavx_replay_sample(ring() if ring_ is None else ring_, count, count_dev, u, rows, s, a_, r, s2, m, tr, en,
                                      ws, ws_bytes, None)

    bad = a.ERR_INVALID_ARG
    assert call(ring_=ctypes.POINTER(a.ReplayRing)()) == bad                                  # NULL ring
    for name in ("obs", "act", "rew", "done"):
        assert call(ring_=ring(**{name: None})) == bad, name
    # the three flag rows are all there or all NULL (packed)
    for miss in (("skip",), ("trunc",), ("ended",), ("skip", "trunc"), ("trunc", "ended"), ("skip", "ended")):
        assert call(ring_=ring(**{n: None for n in miss})) == bad, miss
    for slots in (1, 0, -3, 2 ** 31):
        assert call(ring_=ring(slots=slots)) == bad, slots
    assert call(ring_=ring(envs=0)) == bad and call(ring_=ring(agents=0)) == bad
    for learners in (0, -1, 5):
        assert call(ring_=ring(learners=learners)) == bad, learners
    assert call(ring_=ring(obs=68)) == bad and call(ring_=ring(obs=66)) == bad                # obs not 8-byte aligned
    for count in (0, -1):
        assert call(count=count) == bad, count
    assert call(count=0, count_dev=P + 4) == bad                                              # device count misaligned
    for rows in (-1, 2 ** 20 + 1, 2 ** 40):
        assert call(rows=rows) == bad, rows
    for kw in (dict(u=None), dict(s=None), dict(a_=None), dict(r=None), dict(s2=None), dict(m=None)):
        assert call(**kw) == bad, kw
        assert call(rows=256, **kw) == bad, kw
    assert call(tr=None) == bad and call(en=None) == bad                                      # both or neither
    assert call(s=68) == bad and call(s2=68) == bad and call(a_=68) == bad
    need = ctypes.c_int64()
    assert lib.uavx_replay_workspace_bytes(2048, ctypes.byref(need)) == a.OK
    assert call(ws=None) == bad and call(ws_bytes=need.value - 1) == bad and call(ws_bytes=0) == bad
    assert call(ws=P + 8) == bad                                                              # workspace not 16-byte aligned
    # rows = 0 enqueues nothing and looks at no buffer
    assert call(rows=0, u=None, s=None, ws=None, ws_bytes=0) == a.OK
    assert call(rows=0, tr=None) == a.OK and call(rows=0, en=None) == a.OK      # nor at the pair of flag outputs
    assert call(rows=0, ring_=ring(slots=1)) == bad


def test_replay_kernels_within_budget():
    rows = _kernels()
    # the one-step instantiations of the shared sampler kernels: what uavx_replay_sample launches
    mine = [r for r in rows if r["name"].startswith("uavx_replay_k::")
            and re.search(r"sample_(small|gather)<1, |sample_draw$", r["name"])]
    assert sorted(r["name"].split("::")[1] for r in mine) == [
        "sample_draw", "sample_gather<1, false>", "sample_gather<1, true>", "sample_small<1, false>",
        "sample_small<1, true>"], sorted(r["name"] for r in rows if r["name"].startswith("uavx_replay_k::"))
    for r in mine:
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["private_segment_fixed_size"] == 0, r
        assert r["group_segment_fixed_size"] <= 8192, r
        assert r["agpr_count"] == 0 and r["vgpr_count"] <= 64, r
    # nothing of the new unit is counted among the pinned namespaces
    assert sum(r["name"].startswith("uavx_critic_grad_k::") for r in rows) == 5      # grad_combine, and each tile of grad_rows unweighted and weighted
    assert sum(r["name"].startswith("uavx_optim_k::") for r in rows) == 3
    assert not any("critic_fwd<" in r["name"] or "actor_fwd<" in r["name"] for r in mine)


# ---- the numpy reference against the torch expressions of DeviceReplay.sample ----------------------------------------

L_, E_, N_, T_ = 6, 8, 4, 5


def _ring(seed, skip_rate, packed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn((L_, E_, N_, 10), generator=g)
    act = torch.rand((L_, E_, N_, 2), generator=g) * 2 - 1
    rew = torch.randn((L_, E_, N_), generator=g)
    done = (torch.rand((L_, E_, N_), generator=g) < 0.3).to(torch.uint8)
    skip = (torch.rand((L_, E_), generator=g) < skip_rate).to(torch.uint8)
    trunc = (torch.rand((L_, E_), generator=g) < 0.4).to(torch.uint8)
    ended = (torch.rand((L_, E_), generator=g) < 0.5).to(torch.uint8)
    if packed:
        done[:, :, 0] |= skip * 2 + trunc * 8 + ended * 4
        return dict(obs=obs, act=act, rew=rew, done=done, skip=None, trunc=None, ended=None)
    return dict(obs=obs, act=act, rew=rew, done=done, skip=skip, trunc=trunc, ended=ended)


class _CpuReplay:
    """replay.py:74-79 and :104-133 on CPU tensors, the uniforms handed in (r1, r2 = the two torch.rand((3, B)))."""

    def __init__(self, ring, count, num_learners):
        self.__dict__.update(ring)
        self.packed = ring["skip"] is None
        self.count, self.T, self.L, self.num_learners = count, T_, L_, num_learners

    def _flags(self, s, e):
        if self.packed:
            b = self.done[s, e, 0]
            return (b & 2) != 0, (b & 8) != 0, (b & 4) != 0
        return self.skip[s, e] != 0, self.trunc[s, e] != 0, self.ended[s, e] != 0

    def sample(self, batch_size, draws):
        E, N = E_, self.num_learners
        lo = max(0, self.count - self.T)
        span = self.count - lo
        draws = iter(draws)

        def draw():
            r = next(draws)
            k = lo + (r[0] * span).long().clamp_(max=span - 1)   # k in [lo, count - 1]: only written slots
            return k, (r[1] * E).long().clamp_(max=E - 1), (r[2] * N).long().clamp_(max=N - 1)

        k, e, i = draw()
        k2, e2, i2 = draw()  # one redraw for rows that hit a reset step (rare: one per episode per env)
        bad = self._flags(k % self.L, e)[0]
        k, e, i = torch.where(bad, k2, k), torch.where(bad, e2, e), torch.where(bad, i2, i)
        valid = ~self._flags(k % self.L, e)[0]
        pos = torch.arange(batch_size)
        before = torch.cummax(torch.where(valid, pos, torch.full_like(pos, -1)), dim=0).values
        after = torch.flip(torch.cummin(torch.flip(torch.where(valid, pos, torch.full_like(pos, batch_size)), [0]), dim=0).values, [0])
        src = torch.where(before >= 0, before, after.clamp(max=batch_size - 1))
        k, e, i = k[src], e[src], i[src]
        s, s1 = k % self.L, (k + 1) % self.L
        out = (self.obs[s, e, i], self.act[s, e, i], self.rew[s, e, i], self.obs[s1, e, i],
               1.0 - (self.done[s, e, i] & 1).float())
        _, tr, en = self._flags(s, e)
        return out + (tr, en, src)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("skip_rate", [0.25, 0.9, 1.0])
def test_reference_equals_torch_expressions(skip_rate, packed):
    ring = _ring(int(skip_rate * 100) + packed, skip_rate, packed)
    arrays = {k: (None if v is None else v.numpy()) for k, v in ring.items()}
    g = torch.Generator().manual_seed(11)
    fallbacks = 0
    for count in (1, 3, T_, T_ + 1, 14):                      # below, at and past the horizon (the ring wraps)
        for learners in (4, 3):
            for B in (1, 5, 64, 300):
                r1, r2 = torch.rand((3, B), generator=g), torch.rand((3, B), generator=g)
                want = _CpuReplay(ring, count, learners).sample(B, (r1, r2))
                got = replay_ref.sample(torch.stack((r1, r2)).numpy(), count=count, T=T_, num_learners=learners, **arrays)
                assert len(got) == len(want) == 8
                for x, w in zip(got, want):
                    w = w.numpy()
                    assert x.shape == w.shape and x.dtype == w.dtype and np.array_equal(x, w)
                fallbacks += int((got[7] != np.arange(B)).sum())
                if skip_rate == 1.0:
                    assert (got[7] == B - 1).all()
    assert fallbacks > 0 or skip_rate < 0.5


def test_reference_source_rows_by_hand():
    v = lambda s: np.array([c == "1" for c in s])
    src = replay_ref.source_rows
    assert src(v("0001101")).tolist() == [3, 3, 3, 3, 4, 4, 6]          # invalid run at the start takes the first valid
    assert src(v("1101000")).tolist() == [0, 1, 1, 3, 3, 3, 3]          # invalid run at the end takes the last valid
    assert src(v("00000")).tolist() == [4, 4, 4, 4, 4]                  # no valid row: the last row
    assert src(v("0001000")).tolist() == [3, 3, 3, 3, 3, 3, 3]          # a single valid row in the middle
    assert src(v("1")).tolist() == [0] and src(v("0")).tolist() == [0]
    assert src(v("1111")).tolist() == [0, 1, 2, 3]


def test_reference_out_of_range_uniforms():
    u = np.array([1.0, -0.5, np.nan, np.inf, -np.inf, 1 - 2.0 ** -24, 0.0, 0.999, -0.0, 3e38], dtype=np.float32)
    for n in (1, 3, 8, 5):
        assert replay_ref.pick(u, n).tolist() == [n - 1, 0, 0, n - 1, 0, n - 1, 0, int(np.float32(0.999) * np.float32(n)), 0, n - 1]


def test_fused_replay_sampler_refuses_on_the_host():
    from gym_uav_collision_avoidance_amd.fused_replay import FusedReplaySampler
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    for other in (object(), None, {"obs": 1}, torch.zeros(3)):
        with pytest.raises(TypeError, match="uavx: FusedReplaySampler takes a DeviceReplay"):
            FusedReplaySampler(other)
    mem = DeviceReplay.__new__(DeviceReplay)                   # a ring on the CPU: there is no CPU path
    mem.obs = torch.zeros((L_, E_, N_, 10))
    with pytest.raises(ValueError, match="uavx: .*no CPU path"):
        FusedReplaySampler(mem)
    for rows in (-1, 2 ** 20 + 1):
        with pytest.raises(ValueError, match="uavx: FusedReplaySampler takes 0..1048576 rows"):
            FusedReplaySampler._rows(rows)
    assert FusedReplaySampler._rows(256) == 256

"""Host-side checks of prioritized n-step replay (libuavx_keywalk.so, include/uavx_keywalk.h): the library
builds for gfx950 without a GPU and carries its source hash, exports exactly the two symbols its header declares, refuses
every bad argument before touching a device, its kernels are the 16 walk_rows instantiations without scratch, spills or LDS,
the four other libraries keep the source hashes they had, the numpy restatement the GPU tests trust (keywalk_ref.py) gives
nstep_ref.sample's batches bit for bit, the crafted rings (keywalk_layouts.py) hold every case the GPU tests count on, and
the Python layer refuses what it must without a device."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import keywalk_layouts as kl
import keywalk_ref
import nstep_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _xlib():
    from gym_uav_collision_avoidance_amd import _keywalk_lib
    _keywalk_lib.build()
    return _keywalk_lib


def _kernels():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr.kernel_table(_xlib().LIB_PATH)


# ---- the library ----------------------------------------------------------------------------------------------------------

def test_library_cross_compiles_and_carries_its_source_hash():
    x = _xlib()
    assert os.path.basename(x.LIB_PATH) == "libuavx_keywalk.so" and os.path.isfile(x.LIB_PATH)
    assert x.HEADER == os.path.join(ROOT, "include", "uavx_keywalk.h") and x.HEADER in x._sources()
    assert any(f.endswith(os.path.join("keywalk_csrc", "uavx_keywalk.hip")) for f in x._sources())
    # every file the source includes is under the hash
    src = open(os.path.join(x.CSRC, "uavx_keywalk.hip")).read()
    names = {os.path.basename(f) for f in x._sources()}
    shared = ["uavx_entry.hpp", "uavx_replay_ring.hpp", "uavx_replay_walk.hpp"]
    todo, seen = ["uavx_keywalk.h"] + shared, set()
    assert re.findall(r'#include "([^"]+)"', src) == ["../../include/uavx_keywalk.h"] + [f"../common_csrc/{h}" for h in shared]
    by_name = {os.path.basename(f): f for f in x._sources()}
    while todo:
        h = todo.pop()
        if h in seen:
            continue
        seen.add(h)
        assert h in names, h
        todo += [os.path.basename(i) for i in re.findall(r'#include "([^"]+)"', open(by_name[h]).read())]
    assert seen == {"uavx_keywalk.h", "uavx_replay.h", "uavx_actor.h"} | set(shared)
    blob = open(x.LIB_PATH, "rb").read()
    assert f"UAVX_KEYWALK_SRC_HASH={x.source_hash()}".encode() + b"\0" in blob and b"gfx950" in blob
    assert x._up_to_date()
    mk = open(os.path.join(x.CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, re.M).group(1)
    actor_mk = open(os.path.join(ROOT, "gym_uav_collision_avoidance_amd", "actor_csrc", "Makefile")).read()
    assert flags == re.search(r"^HIPFLAGS \?= (.*)$", actor_mk, re.M).group(1)
    assert "UAVX_KEYWALK_SRC_HASH" in mk and "OUT ?= libuavx_keywalk.so" in mk and "SRCHASH ?=" in mk
    assert "libuavx_keywalk.so.tmp*" in open(os.path.join(ROOT, ".gitignore")).read().split()


def test_library_exports_exactly_what_the_header_declares():
    x = _xlib()
    hdr = open(x.HEADER).read()
    declared = set(re.findall(r"\b(uavx_keywalk[a-z_0-9]*)\s*\(", hdr))
    assert declared == set(x.SYMBOLS) == {"uavx_keywalk_version", "uavx_keywalk"}
    assert x.SYMBOLS[0] == "uavx_keywalk_version"
    lib = x.load()
    assert lib.uavx_keywalk_version() == x.ABI_VERSION == 1 and "#define UAVX_KEYWALK_VERSION 1" in hdr
    # the C symbols the dynamic table defines are those two: nothing else of the ABI's name space leaks out
    out = subprocess.run(["nm", "-D", "--defined-only", x.LIB_PATH], capture_output=True, text=True, check=True).stdout
    c_names = {l.split()[-1] for l in out.splitlines() if " T " in l and not l.split()[-1].startswith("_")}
    assert c_names == declared, c_names
    from gym_uav_collision_avoidance_amd import _actor_lib, _prio_lib
    assert f"#define UAVX_KEYWALK_MAX_ROWS {x.MAX_ROWS}" in hdr and x.MAX_ROWS == _prio_lib.MAX_ROWS == 1048576
    assert f"#define UAVX_KEYWALK_MAX_STEP {x.MAX_STEP}" in hdr and x.MAX_STEP == _actor_lib.NSTEP_MAX == 8
    # the struct the binding fills has the header's fields, in its order
    body = re.search(r"typedef struct uavx_keywalk_args \{(.*?)\} uavx_keywalk_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", d).group(1) for d in body.split(";") if d.strip()]
    assert fields == [n for n, _ in x.Args._fields_]
    assert ctypes.sizeof(x.Args) == 13 * 8


def test_the_other_libraries_keep_their_source_hashes():
    """The constraint this library exists for: nothing the three other libraries are built from has changed since, but for the
    actor library's critic-gradient unit, which took in the weighted gradient (a056e385b4f6651e and ten units before), and for
    what the three replay units had alike, which went to common_csrc/ (17c0e2c29cadcdb4 and 3e2046d3591a64b0 before): no file
    of keywalk_csrc/ is among the others' sources."""
    from gym_uav_collision_avoidance_amd import _actor_lib, _lib, _prio_lib
    assert _actor_lib.source_hash() == "c6725b15f59f1983" and len(_actor_lib.UNITS) == 11
    assert _prio_lib.source_hash() == "75c3f7d1033d0f00"
    assert _lib.source_hash() == "c85b3516db0d8e1b"
    x = _xlib()
    for other in (_actor_lib, _prio_lib):
        assert not any("keywalk" in os.path.basename(f) for f in other._sources())
    assert x.CSRC == os.path.join(ROOT, "gym_uav_collision_avoidance_amd", "keywalk_csrc")


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

    def walk(**kw):
        a = x.Args(ring=ring(), count=3, count_dev=None, key=P, rows=256, n_step=3, gamma=0.99, reward=P, next_state=P,
                   mask=P, length=P, truncated=P, ended=P)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.uavx_keywalk(ctypes.byref(a), None)

    # what is checked with rows = 0 as well: the ring, the count, n_step and gamma
    always = [dict(ring=ctypes.POINTER(x.ReplayRing)())]
    always += [dict(ring=ring(**{name: None})) for name in ("obs", "act", "rew", "done")]
    always += [dict(ring=ring(**{n: None for n in miss})) for miss in
               (("skip",), ("trunc",), ("ended",), ("skip", "trunc"), ("trunc", "ended"), ("skip", "ended"))]
    always += [dict(ring=ring(slots=s)) for s in (1, 0, -3, 2 ** 31)]
    always += [dict(ring=ring(envs=0)), dict(ring=ring(envs=2 ** 31)), dict(ring=ring(agents=0)), dict(ring=ring(agents=2 ** 31))]
    always += [dict(ring=ring(learners=n)) for n in (0, -1, 5)]
    always += [dict(ring=ring(obs=68)), dict(ring=ring(act=68)), dict(ring=ring(rew=66))]
    # sizes whose product overflows: envs·learners past 2^31 − 1, and an observation array past 2^63 bytes
    always += [dict(ring=ring(envs=2 ** 16, agents=2 ** 15, learners=2 ** 15)),
               dict(ring=ring(slots=2 ** 31 - 1, envs=2 ** 31 - 1, agents=2 ** 31 - 1, learners=1)),
               dict(ring=ring(slots=2 ** 31 - 1, envs=2 ** 31 - 1, agents=2 ** 31 - 1, learners=2 ** 31 - 1))]
    always += [dict(count=0), dict(count=-1), dict(count=0, count_dev=P + 4)]
    always += [dict(n_step=n) for n in (0, -1, 9, 2 ** 31 - 1)]
    always += [dict(gamma=g) for g in (float("nan"), float("inf"), -float("inf"), -1e-9, 1.0 + 1e-9, 2.0)]
    for kw in always:
        assert walk(**kw) == bad, kw
        assert walk(rows=0, **kw) == bad, kw
    assert lib.uavx_keywalk(None, None) == bad
    for rows in (-1, 2 ** 20 + 1, 2 ** 40):
        assert walk(rows=rows) == bad, rows
    for name in ("key", "reward", "next_state", "mask"):
        assert walk(**{name: None}) == bad, name
    assert walk(key=68) == bad and walk(next_state=68) == bad and walk(reward=66) == bad and walk(mask=66) == bad
    assert walk(truncated=None) == bad and walk(ended=None) == bad
    assert walk(rows=0, truncated=None) == bad and walk(rows=0, ended=None) == bad
    # rows = 0 enqueues nothing and looks at no buffer; the edges of the ranges are accepted
    assert walk(rows=0, key=None, reward=None, next_state=None, mask=None, length=None) == x.OK
    assert walk(rows=0, truncated=None, ended=None) == x.OK
    for kw in (dict(gamma=0.0), dict(gamma=1.0), dict(n_step=1), dict(n_step=8), dict(count=0, count_dev=P),
               dict(ring=ring(skip=None, trunc=None, ended=None)), dict(ring=ring(envs=2 ** 16, agents=2 ** 15, learners=2 ** 14))):
        assert walk(rows=0, **kw) == x.OK, kw


NAMES = [f"walk_rows<{n}, {p}>" for p in ("false", "true") for n in range(1, 9)]
# kernel -> VGPRs as DESIGN.md §25 documents them; no kernel has LDS
DOCUMENTED = dict(zip(NAMES, (20, 32, 38, 44, 50, 54, 60, 66, 20, 32, 38, 44, 48, 54, 60, 60)))


def test_kernels_are_the_sixteen_walks_without_scratch_spills_or_lds():
    rows = _kernels()
    assert sorted(r["name"] for r in rows) == sorted(f"uavx_keywalk_k::{n}" for n in NAMES)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for r in rows:
        name = r["name"].split("::")[1]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, r
        assert r["agpr_count"] == 0 and r["vgpr_count"] <= DOCUMENTED[name], r
        assert f"| `{name}` | 0 | {DOCUMENTED[name]} |" in design, name


# ---- the restatement against the one DESIGN.md §22 proved -----------------------------------------------------------------------

def _as_walk(lay, u, n_step, gamma):
    """nstep_ref.sample on uniforms u, and keywalk_ref.walk on the keys of the start rows it reports."""
    want = nstep_ref.sample(u, act=lay.act, count=lay.count, T=lay.T, num_learners=lay.learners, n_step=n_step, gamma=gamma,
                            **kl.ring(lay))
    key = (want.k * (kl.E * lay.learners) + want.e * lay.learners + want.i).astype(np.int64)
    got = keywalk_ref.walk(key, count=lay.count, T=lay.T, num_learners=lay.learners, n_step=n_step, gamma=gamma, **kl.ring(lay))
    return want, got


def _same(want, got):
    assert got.live.all()
    for name in ("reward", "next_state", "mask", "truncated", "ended", "length", "reason", "k", "e", "i"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), name


def _cell_uniforms(lay):
    """u [2, 3, rows] whose row j draws cell j of the window x envs x learners, both draws alike."""
    c, lo, span, per = kl.window(lay)
    kk, e, i = np.meshgrid(np.arange(span), np.arange(kl.E), np.arange(lay.learners), indexing="ij")
    u = np.empty((2, 3, kk.size), dtype=np.float32)
    u[:, 0], u[:, 1], u[:, 2] = (kk.ravel() + 0.5) / span, (e.ravel() + 0.5) / kl.E, (i.ravel() + 0.5) / lay.learners
    return u


@pytest.mark.parametrize("gamma", [0.99, 1.0])
@pytest.mark.parametrize("n_step", [1, 2, 3, 8])
@pytest.mark.parametrize("packed", [False, True])
def test_restatement_gives_the_nstep_restatements_batches(packed, n_step, gamma):
    rng = np.random.default_rng(7 * n_step + packed)
    for T in kl.HORIZONS:
        for name in kl.COUNTS:
            for learners in (kl.N, 3):
                lay = kl.craft(T, kl.count_of(name, T), packed, seed=n_step, learners=learners)
                _same(*_as_walk(lay, _cell_uniforms(lay), n_step, gamma))                 # crafted: every cell of the window
                _same(*_as_walk(lay, rng.random((2, 3, 257), dtype=np.float32), n_step, gamma))


# ---- the crafted rings hold what the GPU tests count on --------------------------------------------------------------------------

@pytest.mark.parametrize("n_step", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("name", kl.COUNTS)
@pytest.mark.parametrize("T", kl.HORIZONS)
@pytest.mark.parametrize("packed", [False, True])
def test_crafted_layouts_reach_every_stop_reason_length_and_ignored_kind(packed, T, name, n_step):
    lay = kl.craft(T, kl.count_of(name, T), packed, seed=n_step)
    c, lo, span, per = kl.window(lay)
    key = kl.keys(lay)
    ign = kl.ignored_keys(lay)
    assert len(key) == span * per + len(ign) <= 9 * 8 * 4 + 5 and len(ign) == 4 + (lo > 0)
    assert len(np.unique(key)) == len(key) and span >= 2
    got = keywalk_ref.walk(key, count=lay.count, T=T, num_learners=lay.learners, n_step=n_step, gamma=0.99, **kl.ring(lay))
    cells = slice(0, span * per)
    assert got.live[cells].all() and not got.live[span * per:].any()
    assert (got.reason[span * per:] == 0).all() and (got.length[span * per:] == 0).all()
    assert (got.reason[cells] != 0).all() and (got.length[cells] >= 1).all()
    # the ignored kinds: negative, below the window, at and far past the head
    live, k, _, _ = keywalk_ref.decode(ign, c, T, kl.E, lay.learners)
    assert not live.any() and (ign < 0).sum() == 2 and int(ign[-2]) // per == c and (lo == 0 or int(ign[2]) // per == lo - 1)
    reason, length = got.reason[cells], got.length[cells]
    for why, bit in nstep_ref.REASONS.items():
        if why == "n_step" and n_step > span:
            assert not (reason & bit).any()
            continue
        assert (reason & bit).any(), why
        if span >= 4 and n_step > 1 and (why != "n_step" or n_step < span):
            assert (reason == bit).any(), why          # with one step, n_step ends every walk: nothing else ends one alone
    assert set(np.unique(length).tolist()) == set(range(1, min(n_step, span) + 1))
    # a start row that is itself a reset row is walked like any other (env 0: all of them)
    e0 = got.e[cells] == 0
    assert e0.any() and (length[e0] == 1).all()
    assert ((reason[e0] & (nstep_ref.SKIP | nstep_ref.HEAD | nstep_ref.N_STEP)) != 0).all()
    # flags that live in agent 0's byte (packed) end walks of rows whose own agent is another
    for bit in (nstep_ref.ENDED, nstep_ref.SKIP):
        assert ((reason & bit != 0) & (got.i[cells] != 0)).any()
    # the −0 column keeps its sign through one step
    if n_step == 1:
        col = (got.e[cells] == 1) & (got.i[cells] == 3)
        assert col.any() and np.signbit(got.reward[cells][col]).all() and (got.reward[cells][col] == 0).all()


def test_one_step_of_the_restatement_is_the_one_step_gather():
    """n_step = 1: reward, next_state and mask are the ring's own values of the key's cell, as uavx_prio_sample writes them."""
    for packed in (False, True):
        lay = kl.craft(5, 13, packed)
        key = kl.cell_keys(lay)
        got = keywalk_ref.walk(key, count=lay.count, T=5, num_learners=lay.learners, n_step=1, gamma=0.99, **kl.ring(lay))
        s, e, i = got.k % 6, got.e, got.i
        assert np.array_equal(got.reward.view(np.uint32), lay.rew[s, e, i].view(np.uint32))
        assert np.array_equal(got.next_state, lay.obs[(s + 1) % 6, e, i])
        assert np.array_equal(got.mask, np.float32(1) - (lay.done[s, e, i] & 1).astype(np.float32))
        assert np.array_equal(got.truncated, lay.trunc[s, e] != 0) and np.array_equal(got.ended, lay.ended[s, e] != 0)


# ---- what the Python layer refuses on the host -----------------------------------------------------------------------------

def test_sampler_and_learner_keywords_refused_on_the_host():
    from gym_uav_collision_avoidance_amd.learners import FusedDDPG, FusedSAC, FusedTD3
    from gym_uav_collision_avoidance_amd.prioritized_nstep import KeyWalk, PrioritizedNStepSampler, check_walk
    from gym_uav_collision_avoidance_amd.prioritized_replay import PrioritizedReplaySampler
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    assert issubclass(PrioritizedNStepSampler, PrioritizedReplaySampler)
    for cls in (KeyWalk, PrioritizedNStepSampler):
        for other in (object(), None, {"obs": 1}, torch.zeros(3)):
            with pytest.raises(TypeError, match=f"uavx: {cls.__name__} takes a DeviceReplay"):
                cls(other)
        mem = DeviceReplay.__new__(DeviceReplay)                   # a ring on the CPU: there is no CPU path
        mem.obs = torch.zeros((6, 4, 3, 10))
        with pytest.raises(ValueError, match=f"uavx: {cls.__name__} needs the ring on a GPU.*no CPU path"):
            cls(mem, n_step=99)                                    # the ring's place is looked at first
    assert check_walk(3, 0.99) == (3, 0.99) and check_walk(1, 0) == (1, 0.0) and check_walk(8, 1) == (8, 1.0)
    for n in (0, 9, -1, 2.0, "3", None):
        with pytest.raises(ValueError, match=r"uavx: KeyWalk takes n_step in 1\.\.8"):
            check_walk(n, 0.99)
    for g in (-0.01, 1.01, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match=r"uavx: W takes a finite gamma in \[0, 1\]"):
            check_walk(3, g, "W")
    # the learners check their keywords before they look for a device
    for cls in (FusedSAC, FusedTD3, FusedDDPG):
        for n in (0, 9, -3, 2.0, "3", None, True):
            with pytest.raises(ValueError, match=rf"uavx: {cls.__name__} takes per_n_step as an integer in 1\.\.8, got {n!r}"):
                cls(device="cpu", prioritized=0.6, per_n_step=n)
        with pytest.raises(ValueError, match=rf"uavx: {cls.__name__} .*per_n_step=3 needs prioritized=alpha"):
            cls(device="cpu", per_n_step=3)
        with pytest.raises(ValueError, match="per_n_step=2 needs prioritized=alpha"):
            cls(device="cpu", n_step=3, per_n_step=2)              # the uniform sampler's n_step does not stand in for it
        with pytest.raises(ValueError, match="goes with n_step=1 and recency=0"):
            cls(device="cpu", prioritized=0.6, n_step=3, per_n_step=3)        # that refusal stays
        for kw in (dict(prioritized=0.6, per_n_step=3), dict(prioritized=0.6, per_n_step=8, per_beta=0.4),
                   dict(prioritized=0.6, per_n_step=1), dict(per_n_step=1)):
            with pytest.raises(ValueError, match="uavx: the learners need a GPU"):
                cls(device="cpu", **kw)

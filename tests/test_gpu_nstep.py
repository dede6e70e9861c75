"""NStepReplaySampler (libuavx_actor.so, include/uavx_nstep.h) on the MI355X: for one step bit-identical to
FusedReplaySampler.sample and DeviceReplay.sample on rings written by a real env; for 2, 3 and 8 steps bit-identical to
tests/nstep_ref.py on crafted rings whose every start row is enumerated (each of the five ways a walk ends, both flag
layouts, counts below, at and past the wrap), on walks across the slot wrap and up to the ring's head, on the fallback
patterns across 1024-row blocks, with recency-weighted draws and uniforms outside [0, 1); through graph capture following
the device count; and through the three learners' n_step / recency keywords."""
import functools

import numpy as np
import pytest
import torch

import learner_ref as lr
import nstep_ref
import replay_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
E, N = 8, 4
ROWS = (1, 63, 64, 65, 256, 1024, 1025, 4099)


def _mem(steps, learners=None, packed=False, seed=3, T=5):
    """A ring written by `steps` real env steps with step_cap=3 and auto-reset: about a quarter of its cells are reset rows."""
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    env = BatchedMultiUAVWorld2D(E, num_agents=N, device=DEV, seed=seed)
    mem = DeviceReplay(env, horizon=T, num_learners=learners, packed_flags=packed)
    mem.begin(env.reset())
    _step(mem, steps, seed)
    return env, mem


def _step(mem, steps, seed=0):
    g = torch.Generator(device=DEV).manual_seed(100 + seed)
    for _ in range(steps):
        mem.action_slot().copy_(torch.rand((E, N, 2), generator=g, device=DEV) * 2 - 1)
        mem.step(polar=True, auto_reset="agent0_done", step_cap=3)


@functools.lru_cache(maxsize=None)
def _crafted_mem(packed, T, learners=None):
    """One env and ring per layout and horizon, shared by the crafted tests: _craft rewrites every tensor of it."""
    return _mem(1, learners=learners, packed=packed, T=T)[1]


def _nstep(mem, **kw):
    from gym_uav_collision_avoidance_amd.fused_replay_nstep import NStepReplaySampler
    return NStepReplaySampler(mem, **kw)


def _arrays(mem):
    a = dict(obs=mem.obs, act=mem.act, rew=mem.rew, done=mem.done)
    if not mem.packed:
        a.update(skip=mem.skip, trunc=mem.trunc, ended=mem.ended)
    return {k: v.cpu().numpy() for k, v in a.items()}


def _check_ref(mem, sampler, u, **kw):
    """All seven outputs and the length against the restatement, bit for bit -> the restatement's Batch."""
    want = nstep_ref.sample(u, count=mem.count, T=mem.T, num_learners=mem.num_learners, n_step=sampler.n_step,
                            gamma=sampler.gamma, recency=sampler.recency, **_arrays(mem))
    got = sampler.sample_from_uniforms(torch.from_numpy(u).to(DEV), with_flags=True, with_length=True, **kw)
    torch.cuda.synchronize()
    assert len(got) == 8
    for name, x, w in zip(want._fields, got, tuple(want[:7]) + (want.length,)):
        x = x.cpu().numpy()
        assert x.shape == w.shape and x.dtype == w.dtype, name
        assert np.array_equal(x.view(np.uint8), w.view(np.uint8)), name
    return want


# ---- 1. one step is the one-step sampler -----------------------------------------------------------------------------------

@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("steps", [3, 14])
def test_one_step_equals_fused_sampler_and_device_replay(steps, packed):
    from gym_uav_collision_avoidance_amd.fused_replay import FusedReplaySampler
    env, mem = _mem(steps, packed=packed)
    one, fused = _nstep(mem, n_step=1, gamma=0.99, recency=0.0), FusedReplaySampler(mem)
    for rows in ROWS:
        g = [torch.Generator(device=DEV).manual_seed(rows) for _ in range(3)]
        want = mem.sample(rows, generator=g[0], with_flags=True)
        mid = fused.sample(rows, generator=g[1], with_flags=True)
        got = one.sample(rows, generator=g[2], with_flags=True, with_length=True)
        assert len(got) == 8 and len(want) == len(mid) == 7
        for x, w, m in zip(got, want, mid):
            assert x.shape == w.shape and x.dtype == w.dtype and x.device == w.device and x.is_contiguous()
            assert torch.equal(x.view(torch.uint8), w.view(torch.uint8)) and torch.equal(x, m)
        assert got[7].dtype == torch.uint8 and bool((got[7] == 1).all())
        tail = [torch.rand(7, generator=x, device=DEV) for x in g]          # the generators advanced alike
        assert torch.equal(tail[0], tail[2]) and torch.equal(tail[1], tail[2])
        five = one.sample(rows, generator=torch.Generator(device=DEV).manual_seed(rows))
        assert len(five) == 5 and all(torch.equal(x, w) for x, w in zip(five, want))
    env.close()


# ---- crafted rings -----------------------------------------------------------------------------------------------------------

def _craft(mem, count, seed=0):
    """Overwrites the ring: unique observation cells, random rewards, and flags by env --
    env 0 every cell a reset row (never a valid start); env 1 clean; env 2 done for agents 1 and 2 at steps c − 1 and c − 3;
    env 3 ended (and truncated) at those steps; env 4 skip at those steps; envs 5.. random done / skip / ended / trunc."""
    L = mem.L
    g = torch.Generator(device=DEV).manual_seed(seed)
    mem.obs.copy_(torch.arange(mem.obs.numel(), device=DEV, dtype=torch.float32).view_as(mem.obs))
    mem.act.copy_(-torch.arange(mem.act.numel(), device=DEV, dtype=torch.float32).view_as(mem.act) - 1)
    mem.rew.copy_(torch.randn(mem.rew.shape, generator=g, device=DEV))
    mem.rew[:, 1, 3] = -0.0                                  # a return of −0 keeps its sign (the outputs are compared as bits)
    done = (torch.rand(mem.done.shape, generator=g, device=DEV) < 0.3).to(torch.uint8)
    skip = (torch.rand((L, E), generator=g, device=DEV) < 0.3).to(torch.uint8)
    ended = (torch.rand((L, E), generator=g, device=DEV) < 0.3).to(torch.uint8)
    trunc = ended & (torch.rand((L, E), generator=g, device=DEV) < 0.5).to(torch.uint8)
    done[:, :5], skip[:, :5], ended[:, :5], trunc[:, :5] = 0, 0, 0, 0
    skip[:, 0] = 1
    for step in (count - 1, count - 3):
        if step >= 0:
            s = step % L
            done[s, 2, 1:3], ended[s, 3], trunc[s, 3], skip[s, 4] = 1, 1, 1, 1
    if mem.packed:
        done[:, :, 0] |= skip * 2 + trunc * 8 + ended * 4
        for t in (mem.skip, mem.trunc, mem.ended):
            t.fill_(255)                                     # the packed layout reads none of them
    else:
        mem.skip.copy_(skip), mem.trunc.copy_(trunc), mem.ended.copy_(ended)
    mem.done.copy_(done)
    mem.count = count


def _cells(mem, steps=None, envs=None):
    """u [2, 3, rows] whose row j draws cell j of (steps of the window) x envs x learners, both draws alike."""
    lo = max(0, mem.count - mem.T)
    span = mem.count - lo
    steps = range(span) if steps is None else [k - lo for k in steps]
    envs = range(E) if envs is None else envs
    kk, e, i = np.meshgrid(np.asarray(list(steps)), np.asarray(list(envs)), np.arange(mem.num_learners), indexing="ij")
    u = np.empty((2, 3, kk.size), dtype=np.float32)
    u[:, 0], u[:, 1], u[:, 2] = (kk.ravel() + 0.5) / span, (e.ravel() + 0.5) / E, (i.ravel() + 0.5) / mem.num_learners
    return u, lo + kk.ravel(), e.ravel(), i.ravel()


def _skip_np(mem):
    return ((mem.done[:, :, 0] & 2) != 0).cpu().numpy() if mem.packed else (mem.skip != 0).cpu().numpy()


def _slot_of(state, mem):
    """obs cells are arange: (slot, env, agent) a state row came from."""
    cell = (state[:, 0] // 10).astype(np.int64)
    return cell // (E * N), cell // N % E, cell % N


# ---- 2. every start row of a ring ---------------------------------------------------------------------------------------------

# T = 5 and 7; 9 as well for eight steps, the only horizon here at which a walk can end BY its eighth step, and for 4 to 7
# steps, which have kernels of their own like every n_step
@pytest.mark.parametrize("gamma", [0.99, 1.0])
@pytest.mark.parametrize("T,n_step", [(5, 2), (5, 3), (5, 8), (7, 2), (7, 3), (7, 8), (9, 8), (9, 4), (9, 5), (9, 6), (9, 7)])
@pytest.mark.parametrize("count_of", ["2", "T", "T+1", "2T+3"])
@pytest.mark.parametrize("packed", [False, True])
def test_every_start_row_enumerated(packed, count_of, T, n_step, gamma):
    """Each of the five stop conditions ends at least one row's walk wherever the window lets it: `n_step` needs a window
    of n_step steps (span >= n_step: never with 8 steps and T <= 7, nor with count = 2 and 3 steps), the others need two
    steps, which every count here has.  With four or more steps in the window each also ends a walk ALONE."""
    mem = _crafted_mem(packed, T)
    count = {"2": 2, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3}[count_of]
    _craft(mem, count, seed=count + n_step)
    span = min(count, T)
    u, k, e, i = _cells(mem)
    assert u.shape[2] == span * E * N <= 1024
    want = _check_ref(mem, _nstep(mem, n_step=n_step, gamma=gamma), u)
    ok = ~_skip_np(mem)[k % mem.L, e]                       # a reset row (all of env 0, some elsewhere) falls back
    assert not ok[e == 0].any() and ok[e == 1].all() and 0.5 < ok.mean() < 0.9
    assert np.array_equal(want.src[ok], np.arange(u.shape[2])[ok]) and (want.src[~ok] != np.arange(u.shape[2])[~ok]).all()
    assert np.array_equal(want.k[ok], k[ok]) and np.array_equal(want.e[ok], e[ok]) and np.array_equal(want.i[ok], i[ok])
    for name, bit in nstep_ref.REASONS.items():
        if name == "n_step" and n_step > span:
            assert not (want.reason & bit).any()
            continue
        assert (want.reason & bit).any(), name
        if span >= 4 and (name != "n_step" or n_step < span):
            assert (want.reason == bit).any(), name
    assert set(np.unique(want.length).tolist()) == set(range(1, min(n_step, span) + 1))
    # flags that live in agent 0's byte (packed) end walks of rows whose own agent is another
    for bit in (nstep_ref.ENDED, nstep_ref.SKIP):
        assert ((want.reason & bit != 0) & (want.i != 0)).any()
    assert (want.truncated & (want.i != 0)).any()
    # an agent parked with done = 1 is one step long and masks the bootstrap; a walk that ends otherwise discounts it
    parked = (want.reason & nstep_ref.DONE != 0) & (want.length == 1)
    assert parked.any() and (want.mask[want.reason & nstep_ref.DONE != 0] == 0).all()
    alive = want.reason & nstep_ref.DONE == 0
    chain = np.cumprod(np.r_[1.0, np.full(7, gamma)])       # gamma^(len − 1) as the chain of float64 products
    assert np.array_equal(want.mask[alive], chain[want.length[alive] - 1].astype(np.float32))
    if n_step > 1:
        cut = (want.reason & nstep_ref.ENDED != 0) & alive & (want.length > 1)
        assert cut.any() and (want.mask[cut] > 0).all()     # a time-limit end mid-walk still bootstraps


# ---- 3. walks across the slot wrap and up to the head -----------------------------------------------------------------------

@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("count", [13, 14, 15, 5])
def test_walks_across_the_slot_wrap_and_to_the_head(count, packed):
    T = 5
    mem = _crafted_mem(packed, T)
    L = mem.L
    _craft(mem, count, seed=count)
    lo = max(0, count - T)
    # the steps in slots L − 1 and L − 2 of the window, and the two newest steps
    steps = sorted({k for k in range(lo, count) if k % L in (L - 1, L - 2)} | {count - 1, count - 2})
    u, k, e, i = _cells(mem, steps=steps, envs=(1, 2, 5))
    want = _check_ref(mem, _nstep(mem, n_step=3, gamma=0.99), u)
    clean = e == 1                                          # nothing but n_step and the head ends a walk in env 1
    assert np.array_equal(want.length[clean], np.minimum(3, count - k[clean]))
    slot, env, agent = _slot_of(want.next_state, mem)
    assert np.array_equal(slot, (want.k + want.length) % L) and np.array_equal(env, want.e) and np.array_equal(agent, want.i)
    if count > T:
        wrapped = (want.k % L) + want.length >= L
        assert wrapped[clean].any() and (slot[wrapped & clean] < 3).all()
    rew = mem.rew.cpu().numpy().astype(np.float64)
    for j in np.flatnonzero(clean):
        R, g = -0.0, 1.0
        for t in range(int(want.length[j])):
            R, g = R + g * rew[(k[j] + t) % L, 1, i[j]], g * 0.99
        assert want.reward[j] == np.float32(R)
    newest = want.k == count - 1
    assert newest.any() and (want.length[newest] == 1).all() and (want.reason[newest] & nstep_ref.HEAD != 0).all()


# ---- 4. redraw and fallback with a walk -------------------------------------------------------------------------------------

def _uniforms5(rows, invalid, seed=0, redrawn=()):
    """u [2, 5, rows]: rows of `invalid` draw env 0 twice, rows of `redrawn` draw it once, every other row never."""
    rng = np.random.default_rng(seed)
    u = rng.random((2, 5, rows), dtype=np.float32)
    u[:, 1] = (rng.integers(1, E, size=(2, rows)) + 0.5) / E
    inv = np.asarray(list(invalid), dtype=np.int64)
    u[0, 1, inv] = u[1, 1, inv] = 0.5 / E
    u[0, 1, np.asarray(list(redrawn), dtype=np.int64)] = 0.25 / E
    return u


FALLBACK = {
    "none_valid": lambda rows: range(rows),
    "only_first_valid": lambda rows: range(1, rows),
    "only_last_valid": lambda rows: range(rows - 1),
    "runs_over_block_edges": lambda rows: [j for j in range(rows) if 1000 <= j < 1101 or 2040 <= j < 3080 or j >= rows - 3],
}


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("rows", [1025, 4099])
@pytest.mark.parametrize("case", sorted(FALLBACK))
def test_fallback_patterns_with_a_walk(case, rows, packed):
    mem = _crafted_mem(packed, 5)
    _craft(mem, count=9, seed=rows)
    # env 0 is all reset rows; envs 4.. hold reset rows of their own, so the draws meant to be valid stay in envs 1..3
    invalid = set(FALLBACK[case](rows))
    redrawn = [j for j in range(3, rows, 7) if j not in invalid]
    u = _uniforms5(rows, invalid, seed=len(case), redrawn=redrawn)
    env13 = ((np.random.default_rng(rows).integers(1, 4, size=(2, rows)) + 0.5) / E).astype(np.float32)
    keep = np.ones(rows, dtype=bool)
    keep[list(invalid)] = False
    u[1, 1, keep] = env13[1, keep]
    plain = keep.copy()
    plain[redrawn] = False
    u[0, 1, plain] = env13[0, plain]
    want = _check_ref(mem, _nstep(mem, n_step=3, gamma=0.99, recency=0.8), u)
    valid = np.array([j not in invalid for j in range(rows)])
    assert np.array_equal(want.src, replay_ref.source_rows(valid))        # the restatement saw the intended pattern
    if case == "none_valid":
        assert (want.src == rows - 1).all()
    if case == "only_first_valid":
        assert (want.src == 0).all()
    if case == "only_last_valid":
        assert (want.src == rows - 1).all()
    if case == "runs_over_block_edges":
        assert (want.src[1000:1101] == 999).all() and (want.src[2040:3080] == 2039).all()
        assert len(set(want.length.tolist())) > 1 and (want.src[-3:] == (999 if rows == 1025 else rows - 4)).all()


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("n_step", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_step_count_in_both_launch_forms(n_step, packed):
    """Every n_step has kernels of its own, one for a single launch and one for the gather launch of a large batch."""
    mem = _crafted_mem(packed, 9)
    _craft(mem, count=30, seed=n_step)
    lengths = set()
    for rows in (700, 1100):
        u = np.random.default_rng(rows + n_step).random((2, 5, rows), dtype=np.float32)
        want = _check_ref(mem, _nstep(mem, n_step=n_step, gamma=0.99, recency=0.8), u)
        assert (want.src != np.arange(rows)).any()
        lengths |= set(want.length.tolist())
    assert lengths == set(range(1, n_step + 1))


# ---- 5. recency ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("recency", [0.0, 0.8, 1.0])
def test_recency_picks_the_restatements_rows(recency, packed):
    mem = _crafted_mem(packed, 7)
    for count in (3, 7, 30):
        _craft(mem, count, seed=count)
        lo = max(0, count - mem.T)
        for rows in (300, 2500):
            u = np.random.default_rng(rows + count).random((2, 5, rows), dtype=np.float32)
            want = _check_ref(mem, _nstep(mem, n_step=2, gamma=0.99, recency=recency), u)
            slot, env, agent = _slot_of(want.state, mem)
            assert np.array_equal(slot, want.k % mem.L) and np.array_equal(env, want.e) and np.array_equal(agent, want.i)
            assert lo <= want.k.min() and want.k.max() < count
            # rows whose first draw is no reset row keep it: the newer of the two indices under the coin, else the first
            skip = _skip_np(mem)
            ka, kb = lo + replay_ref.pick(u[0, 0], count - lo), lo + replay_ref.pick(u[0, 3], count - lo)
            coin = u[0, 4] < np.float32(recency)
            k0 = np.where(coin, np.maximum(ka, kb), ka)
            first = ~skip[k0 % mem.L, replay_ref.pick(u[0, 1], E)]
            assert first.any() and np.array_equal(want.k[first], k0[first])
            assert np.array_equal(want.src[first], np.arange(rows)[first])
            assert coin.any() == (recency > 0) and coin.all() == (recency == 1.0)
            if recency == 1.0 and count == 30:
                assert want.k.mean() > (lo + count - 1) / 2 + 0.5          # the draw leans to the newer steps


@pytest.mark.parametrize("packed", [False, True])
def test_uniforms_outside_the_unit_interval_stay_inside_the_ring(packed):
    """1.0, −0.5, NaN, ±inf and 1 − 2^-24 in every one of the five planes of u: the indices follow the header's rule and
    nothing next to the ring is read -- the ring tensors sit inside larger ones filled with a sentinel."""
    T = 5
    env, mem = _mem(1, learners=3, packed=packed, T=T)
    L = mem.L
    SENT = 7.0e7
    for name in ("obs", "act", "rew", "done", "skip", "trunc", "ended"):
        t = getattr(mem, name)
        big = torch.full((L + 2,) + tuple(t.shape[1:]), 255 if t.dtype == torch.uint8 else SENT, dtype=t.dtype, device=DEV)
        setattr(mem, name, big[1:L + 1])
        assert getattr(mem, name).is_contiguous()
    _craft(mem, count=9)
    special = np.array([1.0, -0.5, np.nan, np.inf, -np.inf, 1 - 2.0 ** -24, 2.5, -1e30, 3e38, -0.0], dtype=np.float32)
    u = _uniforms5(128, range(20, 24), seed=5)
    for d in range(2):
        for c in range(5):
            at = 2 + 10 * (d * 5 + c)
            u[d, c, at:at + 10] = special
    u[:, :, 110:120] = special                                  # and every plane at once
    for recency in (0.8, 1.0):
        sampler = _nstep(mem, n_step=3, gamma=0.99, recency=recency)
        want = _check_ref(mem, sampler, u)
        got = sampler.sample_from_uniforms(torch.from_numpy(u).to(DEV), with_flags=True)
        for x in got[:5]:
            assert bool(torch.isfinite(x).all()) and not bool((x.abs() >= SENT).any())
        assert 0 <= want.k.min() - (9 - T) and want.k.max() < 9 and want.e.max() < E and want.i.max() < 3
    env.close()


# ---- 6. graph capture ---------------------------------------------------------------------------------------------------------

def _allocations():
    return torch.cuda.memory_stats(DEV)["allocation.all.allocated"]


@pytest.mark.parametrize("packed", [False, True])
def test_graph_capture_follows_the_device_count(packed):
    T = 5
    env, mem = _mem(3, packed=packed, T=T)
    B = 2048
    sampler = _nstep(mem, n_step=3, gamma=0.99, recency=0.8).reserve(B)
    u_np = np.random.default_rng(9).random((2, 5, B), dtype=np.float32)        # real reset rows decide validity
    u = torch.from_numpy(u_np).to(DEV)
    bufs = (torch.zeros((B, 10), device=DEV), torch.zeros((B, 2), device=DEV), torch.zeros(B, device=DEV),
            torch.zeros((B, 10), device=DEV), torch.zeros(B, device=DEV), torch.zeros(B, dtype=torch.bool, device=DEV),
            torch.zeros(B, dtype=torch.bool, device=DEV), torch.zeros(B, dtype=torch.uint8, device=DEV))
    scratch = torch.zeros(8, device=DEV)
    sampler.push_count()
    sampler.sample_from_uniforms(u, out=bufs, device_count=True)                # warm-up outside the capture
    scratch.add_(1)
    torch.cuda.synchronize()
    # the allocator's count of allocations (a host-side read) does not move across the captured call
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1)
        n0 = _allocations()
        out = sampler.sample_from_uniforms(u, out=bufs, device_count=True)
        n1 = _allocations()
    assert n1 == n0
    assert [o.data_ptr() for o in out] == [b.data_ptr() for b in bufs]
    for extra in (0, 1, T + 2):                             # count 3, 4 and 11 (wrapped)
        _step(mem, extra, seed=extra)
        sampler.push_count()
        for b in bufs:
            b.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = nstep_ref.sample(u_np, count=mem.count, T=T, num_learners=mem.num_learners, n_step=3, gamma=0.99, recency=0.8,
                                **_arrays(mem))
        for x, w in zip(bufs, tuple(want[:7]) + (want.length,)):
            assert np.array_equal(x.cpu().numpy(), w)
    assert mem.count == 3 + 1 + T + 2 and (want.src != np.arange(B)).any() and len(set(want.length.tolist())) == 3
    # a capture cannot allocate the workspace of a large batch
    fresh = _nstep(mem, n_step=3, gamma=0.99, recency=0.8)
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="uavx: the workspace for 2048 rows must exist before a graph capture"):
        with torch.cuda.graph(g2):
            scratch.add_(1)
            fresh.sample_from_uniforms(u, out=bufs, device_count=True)
    torch.cuda.synchronize()
    env.close()


# ---- 7. learners ----------------------------------------------------------------------------------------------------------------

NETS = {"sac": ("policy", "critic", "critic_target"), "td3": ("actor", "actor_target", "critic", "critic_target"),
        "ddpg": ("actor", "actor_target", "critic", "critic_target")}


def _learner(kind, **kw):
    from gym_uav_collision_avoidance_amd import learners
    cls = {"sac": learners.FusedSAC, "td3": learners.FusedTD3, "ddpg": learners.FusedDDPG}[kind]
    return lr.load_recipe(cls(device=DEV, **kw), kind).refresh()


def _state(agent, kind):
    """Every tensor an update moves, cloned: parameters, targets, optimiser moments, SAC's log_alpha and alpha."""
    out = [p.detach().clone() for k in NETS[kind] for p in getattr(agent, k).parameters()]
    for n in ("critic_optim", "policy_optim", "alpha_optim", "actor_optimizer", "critic_optimizer"):
        opt = getattr(agent, n, None)
        if opt is not None:
            for g in opt.param_groups:
                for p in g["params"]:
                    out += [v.detach().clone() for k, v in sorted(opt.state[p].items()) if k != "step"]
    if kind == "sac":
        out += [agent.log_alpha.detach().clone(), agent.alpha.clone()]
    return out


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), i


@pytest.fixture(scope="module")
def memory():
    env, mem = _mem(40, T=32)
    yield mem
    env.close()


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_learner_keywords_equal_an_explicit_nstep_batch(kind, memory):
    from gym_uav_collision_avoidance_amd.fused_replay import FusedReplaySampler
    from gym_uav_collision_avoidance_amd.fused_replay_nstep import NStepReplaySampler
    B = 64
    gen = lambda: torch.Generator(device=DEV).manual_seed(77)
    a = _learner(kind, generator=gen(), memory=memory, n_step=3, recency=0.8)
    assert type(a._sampler) is NStepReplaySampler and a._sampler.n_step == 3 and a._sampler.recency == 0.8
    assert a._sampler.gamma == 0.99 == (a.discount if kind == "td3" else a.gamma)
    gb = gen()
    b = _learner(kind, generator=gb)
    assert b._sampler is None and type(b.attach(memory)._sampler) is FusedReplaySampler      # the defaults change nothing
    side = NStepReplaySampler(memory, n_step=3, gamma=0.99, recency=0.8)
    lengths = set()
    for _ in range(2):
        a.update_parameters(memory, B)
        batch = side.sample(B, generator=gb, with_length=True)
        assert bool(((batch[4] != 0) & (batch[4] != 1)).any())         # an ordinary batch whose mask is not 0 / 1
        lengths |= set(batch[5].tolist())
        b.update_batch(*batch[:5])
    torch.cuda.synchronize()
    assert lengths == {1, 2, 3}
    _same(_state(a, kind), _state(b, kind))
    la, lb = a.losses(), b.losses()
    assert la.shape == (2, 8) and np.array_equal(la.view(np.int32), lb.view(np.int32))
    # the same through capture / run against the eager pair
    c = _learner(kind, generator=gen(), memory=memory, n_step=3, recency=0.8)
    c.capture(B)
    c.run(2)
    torch.cuda.synchronize()
    _same(_state(c, kind), _state(a, kind))
    assert np.array_equal(c.losses().view(np.int32), la.view(np.int32))
    for x in (a, b, c):
        x.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals(memory):
    from gym_uav_collision_avoidance_amd import learners
    from gym_uav_collision_avoidance_amd.fused_replay_nstep import NStepReplaySampler
    with pytest.raises(TypeError, match="uavx: NStepReplaySampler takes a DeviceReplay, not Tensor"):
        NStepReplaySampler(torch.zeros(3, device=DEV))
    for n in (0, 9, 2.5):
        with pytest.raises(ValueError, match=r"uavx: NStepReplaySampler takes n_step in 1\.\.8, got"):
            NStepReplaySampler(memory, n_step=n)
    for gamma in (0.0, 1.5, -1.0, float("nan")):
        with pytest.raises(ValueError, match=r"uavx: NStepReplaySampler takes gamma in \(0, 1\], got"):
            NStepReplaySampler(memory, gamma=gamma)
    for recency in (-0.5, 1.01):
        with pytest.raises(ValueError, match=r"uavx: NStepReplaySampler takes recency in \[0, 1\], got"):
            NStepReplaySampler(memory, recency=recency)
    B = 256
    s = NStepReplaySampler(memory, n_step=3, gamma=0.99, recency=0.8)
    bufs = (torch.zeros((B, 10), device=DEV), torch.zeros((B, 2), device=DEV), torch.zeros(B, device=DEV),
            torch.zeros((B, 10), device=DEV), torch.zeros(B, device=DEV), torch.zeros(B, dtype=torch.bool, device=DEV),
            torch.zeros(B, dtype=torch.bool, device=DEV), torch.zeros(B, dtype=torch.uint8, device=DEV))
    g = torch.Generator(device=DEV).manual_seed(1)
    state = g.get_state()
    with pytest.raises(ValueError, match="uavx: out must hold 5 tensors"):
        s.sample(B, generator=g, out=bufs[:4])
    with pytest.raises(ValueError, match=r"uavx: out\[state\] must be"):
        s.sample(B, generator=g, out=(bufs[0][:100],) + bufs[1:5])
    with pytest.raises(ValueError, match=r"uavx: out\[length\] must be torch.uint8"):
        s.sample(B, generator=g, out=bufs[:7] + (bufs[2],))
    with pytest.raises(ValueError, match=r"uavx: out\[action\] must be contiguous"):
        s.sample(B, generator=g, out=(bufs[0], torch.zeros((B, 4), device=DEV)[:, :2]) + bufs[2:5])
    with pytest.raises(ValueError, match=r"uavx: out\[mask\] is on cpu"):
        s.sample(B, generator=g, out=bufs[:4] + (torch.zeros(B),))
    with pytest.raises(ValueError, match="uavx: NStepReplaySampler takes 0..1048576 rows"):
        s.sample(2 ** 20 + 1, generator=g)
    with pytest.raises(ValueError, match="uavx: the uniforms must be a float32 tensor of shape"):
        s.sample_from_uniforms(torch.zeros((2, 4, 8), device=DEV))
    with pytest.raises(ValueError, match=r"uavx: recency = 0.8 needs uniforms of shape \[2, 5, rows\]"):
        s.sample_from_uniforms(torch.zeros((2, 3, 8), device=DEV))
    env2, empty = _mem(0)
    with pytest.raises(ValueError, match="uavx: the replay memory is empty"):
        NStepReplaySampler(empty).sample(B, generator=g)
    env2.close()
    assert torch.equal(g.get_state(), state)                # a refused call leaves the generator where it was
    out = s.sample(B, generator=g, out=bufs)                # and all eight buffers are taken
    assert len(out) == 8 and [o.data_ptr() for o in out] == [b.data_ptr() for b in bufs]
    assert s.sample(0, generator=g)[0].shape == (0, 10) and s.workspace_bytes(1024) == 0 < s.workspace_bytes(1025)
    for cls in (learners.FusedSAC, learners.FusedTD3, learners.FusedDDPG):
        with pytest.raises(ValueError, match=rf"uavx: {cls.__name__} takes n_step in 1\.\.8, got 0"):
            cls(device=DEV, n_step=0)
        with pytest.raises(ValueError, match=rf"uavx: {cls.__name__} takes recency in \[0, 1\], got -1"):
            cls(device=DEV, recency=-1)

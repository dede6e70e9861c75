"""Prioritized n-step replay (libuavx_keywalk.so, include/uavx_keywalk.h) on the MI355X, bit for bit against
tests/keywalk_ref.py: the walk launch alone on the crafted rings of keywalk_layouts.py with every key of the window and
every ignored kind, at the edges of the launch grid inside guard-padded outputs, across the slot wrap and up to the head;
PrioritizedNStepSampler against its parent for one step and against prio_ref + keywalk_ref for more, with nothing to
draw, and through a captured graph that follows the device count; and the learners' `per_n_step` keyword, eager against
captured against a learner fed from a stand-alone sampler."""
import types

import numpy as np
import pytest
import torch

import keywalk_layouts as kl
import keywalk_ref
import prio_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
E, N = kl.E, kl.N
ROWS = (1, 63, 64, 65, 1025, 4099)
ONE = prio_ref.ONE
SENTINEL, BYTE = -7.0, 99


def _walk(mem, n_step, gamma):
    from gym_uav_collision_avoidance_amd.prioritized_nstep import KeyWalk
    return KeyWalk(mem, n_step=n_step, gamma=gamma)


def _pern(mem, **kw):
    from gym_uav_collision_avoidance_amd.prioritized_nstep import PrioritizedNStepSampler
    return PrioritizedNStepSampler(mem, **kw)


def _per(mem, **kw):
    from gym_uav_collision_avoidance_amd.prioritized_replay import PrioritizedReplaySampler
    return PrioritizedReplaySampler(mem, **kw)


def _upload(lay):
    """A DeviceReplay that no env wrote: the layout's arrays on the device, and its count."""
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    mem = DeviceReplay.__new__(DeviceReplay)
    mem.env = types.SimpleNamespace(num_envs=E, num_agents=N, device=DEV)
    mem.T, mem.L, mem.num_learners, mem.packed, mem.count = lay.T, lay.T + 1, lay.learners, lay.packed, lay.count
    for name in ("obs", "act", "rew", "done"):
        setattr(mem, name, torch.from_numpy(getattr(lay, name)).to(DEV))
    for name in ("skip", "trunc", "ended"):
        t = torch.from_numpy(getattr(lay, name)).to(DEV)
        setattr(mem, name, torch.full_like(t, 255) if lay.packed else t)      # the packed layout reads none of them
    return mem


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
    g = torch.Generator(device=DEV).manual_seed(100 + seed + mem.count)
    for _ in range(steps):
        mem.action_slot().copy_(torch.rand((E, N, 2), generator=g, device=DEV) * 2 - 1)
        mem.step(polar=True, auto_reset="agent0_done", step_cap=3)


def _arrays(mem):
    a = dict(obs=mem.obs, act=mem.act, rew=mem.rew, done=mem.done)
    if not mem.packed:
        a.update(skip=mem.skip, trunc=mem.trunc, ended=mem.ended)
    return {k: v.cpu().numpy() for k, v in a.items()}


def _ring(arrays):
    return {k: v for k, v in arrays.items() if k != "act"}


def _state(per):
    """(table, record) of a sampler as the restatement takes them."""
    torch.cuda.synchronize()
    return per.priorities.cpu().numpy().copy(), prio_ref.Record(**per.record())


def _guarded(shape, dtype, fill, pad=64):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=DEV)
    return buf, buf[pad:pad + n].view(shape)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


WALKED = ("reward", "next_state", "mask", "truncated", "ended")


def _same_walk(got, want, before=None):
    """got: (reward, next_state, mask, truncated, ended, length) arrays, the flags uint8 or bool.  Rows the restatement
    walked equal it bit for bit; rows it ignored hold what they held `before` (arrays in the same order, or None: the
    sentinels) and have length 0."""
    live = want.live
    for k, name in enumerate(WALKED):
        x, w = got[k], getattr(want, name)
        assert x.shape == w.shape, name
        if x.dtype == np.uint8:                             # a flag as the kernel wrote it: a 0 / 1 byte
            assert w.dtype == np.bool_ and set(np.unique(x[live]).tolist()) <= {0, 1}, name
            assert np.array_equal(x[live] != 0, w[live]), name
        else:
            assert x.dtype == w.dtype and np.array_equal(_bits(x[live]), _bits(w[live])), name
        if before is None:
            assert (x[~live] == (BYTE if x.dtype == np.uint8 else SENTINEL)).all(), name
        else:
            assert x.dtype == before[k].dtype and np.array_equal(_bits(x[~live]), _bits(before[k][~live])), name
    assert got[5].dtype == np.uint8 and np.array_equal(got[5], want.length)
    assert (got[5][~live] == 0).all() and (got[5][live] >= 1).all()


def _check_walk(mem, lay, key, n_step, gamma):
    """KeyWalk.extend on guard-padded, sentinel-filled outputs against the restatement -> the restatement's Walk."""
    rows = len(key)
    want = keywalk_ref.walk(key, count=lay.count, T=lay.T, num_learners=lay.learners, n_step=n_step, gamma=gamma, **kl.ring(lay))
    specs = [((rows,), torch.float32, SENTINEL), ((rows, 10), torch.float32, SENTINEL), ((rows,), torch.float32, SENTINEL),
             ((rows,), torch.uint8, BYTE), ((rows,), torch.uint8, BYTE), ((rows,), torch.uint8, BYTE)]
    guarded = [_guarded(*s) for s in specs]
    r, s2, m, tr, en, ln = (v for _, v in guarded)
    kbuf, kview = _guarded((rows,), torch.int64, -77)
    kview.copy_(torch.from_numpy(key))
    _walk(mem, n_step, gamma).extend(kview, r, s2, m, length=ln, truncated=tr, ended=en)
    torch.cuda.synchronize()
    _same_walk([t.cpu().numpy() for t in (r, s2, m, tr, en, ln)], want)
    for (buf, _), (shape, _, fill) in zip(guarded, specs):
        n = int(np.prod(shape))
        assert bool((buf[:64] == fill).all()) and bool((buf[64 + n:] == fill).all())
    assert bool((kbuf[:64] == -77).all()) and bool((kbuf[64 + rows:] == -77).all()) and torch.equal(kview.cpu(), torch.from_numpy(key))
    return want


# ---- 1. crafted rings, every key ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gamma", [0.99, 1.0])
@pytest.mark.parametrize("T,n_step", [(5, 1), (5, 2), (5, 3), (5, 8), (9, 4), (9, 5), (9, 6), (9, 7), (9, 8)])
@pytest.mark.parametrize("packed", [False, True])
def test_every_key_of_the_crafted_rings(packed, T, n_step, gamma):
    """Every cell of the window and every ignored kind of key, at each of the four counts; test_keywalk_host.py shows that
    these layouts reach every stop reason, every length and every ignored kind."""
    for name in kl.COUNTS:
        lay = kl.craft(T, kl.count_of(name, T), packed, seed=n_step)
        key = kl.keys(lay)
        assert len(key) <= 10 * 8 * 4 + 5
        want = _check_walk(_upload(lay), lay, key, n_step, gamma)
        dead = len(kl.ignored_keys(lay))
        assert want.live[:-dead].all() and not want.live[-dead:].any()


# ---- 2. the edges of the launch grid -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_step", [3, 8])
@pytest.mark.parametrize("packed", [False, True])
def test_grid_edges_inside_guarded_outputs(packed, n_step):
    lay = kl.craft(9, 21, packed, seed=n_step)
    mem = _upload(lay)
    cells, dead = kl.cell_keys(lay), kl.ignored_keys(lay)
    rng = np.random.default_rng(n_step)
    for rows in ROWS:
        key = rng.choice(cells, size=rows, replace=True)
        if rows > 64:
            key[[0, 63, 64, rows - 1]] = dead[[0, 1, 2, 3]]       # ignored rows at the edges of waves and of the grid
        want = _check_walk(mem, lay, key, n_step, 0.99)
        assert len(set(want.length.tolist())) > 1 or rows == 1


# ---- 3. walks across the slot wrap and up to the head --------------------------------------------------------------------------

@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("T,count", [(7, 13), (7, 14), (7, 15), (5, 5)])
def test_walks_across_the_slot_wrap_and_to_the_head(T, count, packed):
    lay = kl.craft(T, count, packed, seed=count, learners=3)       # three learners of four agents: keys count learners
    L = T + 1
    want = _check_walk(_upload(lay), lay, kl.cell_keys(lay), 3, 0.99)
    assert want.live.all()
    clean = want.e == 1                                        # nothing but n_step and the head ends a walk in env 1
    assert np.array_equal(want.length[clean], np.minimum(3, count - want.k[clean]))
    cell = (want.next_state[:, 0] // 10).astype(np.int64)      # obs cells are arange: where a next_state row came from
    assert np.array_equal(cell // (E * N), (want.k + want.length) % L)
    assert np.array_equal(cell // N % E, want.e) and np.array_equal(cell % N, want.i) and want.i.max() == 2
    # counts 13 and 14 put slot L − 1 inside the window, so walks cross the wrap; at 15 the window starts in slot 0 and the
    # head is slot L − 1: nothing wraps, and lo % slots is 0
    wrapped = (want.k % L) + want.length >= L
    if (np.arange(max(0, count - T), count) % L == L - 1).any():
        assert count in (13, 14) and wrapped[clean].any() and (cell[wrapped & clean] // (E * N) < 3).all()
    else:
        assert count in (15, 5) and not wrapped.any()
    newest = want.k == count - 1
    assert newest.any() and (want.length[newest] == 1).all() and (cell[newest] // (E * N) == count % L).all()   # the head slot


# ---- 4. one step through the new class is the parent ---------------------------------------------------------------------------

@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("steps", [3, 14])
def test_one_step_equals_the_prioritized_sampler(steps, packed):
    env, mem = _mem(steps, packed=packed)
    table = torch.from_numpy(np.random.default_rng(steps).integers(1, 2 ** 20, (mem.L, E, N), dtype=np.int64).astype(np.int32))
    one, parent = _pern(mem, n_step=1, gamma=0.99, alpha=1.0), _per(mem, alpha=1.0)
    one.set_priorities(table), parent.set_priorities(table)
    for rows in ROWS:
        g = [torch.Generator(device=DEV).manual_seed(rows) for _ in range(2)]
        want = parent.sample(rows, generator=g[0], with_flags=True)
        got = one.sample(rows, generator=g[1], with_flags=True, with_length=True)
        assert len(want) == 9 and len(got) == 10
        for x, w in zip(got, want):
            assert x.shape == w.shape and x.dtype == w.dtype and x.device == w.device and x.is_contiguous()
            assert torch.equal(x.view(torch.uint8), w.view(torch.uint8))
        assert bool((got[6] >= 0).all()) and got[9].dtype == torch.uint8 and bool((got[9] == 1).all())
        assert torch.equal(torch.rand(7, generator=g[0], device=DEV), torch.rand(7, generator=g[1], device=DEV))
        seven = one.sample(rows, generator=torch.Generator(device=DEV).manual_seed(rows))
        assert len(seven) == 7 and all(torch.equal(x, w) for x, w in zip(seven, want))
    assert torch.equal(one.priorities.view(torch.int32), parent.priorities.view(torch.int32)) and one.record() == parent.record()
    env.close()


# ---- 5. the full sampler ---------------------------------------------------------------------------------------------------------

def _expect(per, state, mem, u, arrays):
    """What refresh + draw + walk give on the uniforms u from the sampler state (table, record) -> (table, record, draw, walk)."""
    table, rec = prio_ref.refresh(state[0], state[1], mem.count, arrays["done"], arrays.get("skip"))
    draw = prio_ref.sample(u, table, rec, mem.count, stratified=per.stratified, beta=per.beta, **arrays)
    want = keywalk_ref.walk(draw.key, count=mem.count, T=mem.T, num_learners=mem.num_learners, n_step=per.n_step,
                            gamma=per.gamma, **_ring(arrays))
    return table, rec, draw, want


def _compare(got, draw, want, beta):
    """The ten outputs: state, action, weight, key against prio_ref, the rest against keywalk_ref."""
    assert len(got) == 10
    got = [t.cpu().numpy() for t in got]
    for k, name in ((0, "state"), (1, "action"), (6, "key")):
        w = getattr(draw, name)
        assert got[k].shape == w.shape and got[k].dtype == w.dtype and np.array_equal(_bits(got[k]), _bits(w)), name
    # the weight is one float64 pow rounded once to float32 on both sides: at most one float32 ulp apart (exact at beta = 0)
    a, b = got[5].view(np.int32).astype(np.int64), draw.weight.view(np.int32).astype(np.int64)
    assert got[5].dtype == np.float32 and int(np.abs(a - b).max()) <= (0 if beta == 0.0 else 1)
    before = [draw.reward, draw.next_state, draw.mask, draw.truncated, draw.ended]
    _same_walk([got[2], got[3], got[4], got[7], got[8], got[9]], want, before=before)


def _check_sampler(per, mem, u, arrays):
    """sample_from_uniforms against the restatements: the table, the record and every output -> (draw, walk)."""
    table, rec, draw, want = _expect(per, _state(per), mem, u, arrays)
    got = per.sample_from_uniforms(torch.from_numpy(u).to(DEV), with_flags=True, with_length=True)
    got_table, got_rec = _state(per)
    assert np.array_equal(got_table, table) and got_rec == rec
    _compare(got, draw, want, per.beta)
    return draw, want


@pytest.mark.parametrize("n_step", [3, 8])
@pytest.mark.parametrize("packed", [False, True])
def test_full_sampler_on_a_real_ring(packed, n_step):
    env, mem = _mem(14, packed=packed)
    per = _pern(mem, n_step=n_step, gamma=0.99, alpha=0.6, beta=0.4)
    rng = np.random.default_rng(n_step)
    per.set_priorities(torch.from_numpy(rng.integers(1, 2 ** 20, (mem.L, E, N), dtype=np.int64).astype(np.int32)))
    arrays = _arrays(mem)
    lengths = set()
    for rows in (257, 1025):
        draw, want = _check_sampler(per, mem, rng.random(rows, dtype=np.float32), arrays)
        assert want.live.all() and (draw.key >= 0).all()
        lengths |= set(want.length.tolist())
    assert {1, 2} <= lengths <= {1, 2, 3}                          # step_cap=3: no episode is longer than three steps
    env.close()


# ---- 6. nothing to draw ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("packed", [False, True])
def test_total_zero_keeps_the_one_step_outputs(packed):
    lay = kl.craft(5, 9, packed)
    lay = lay._replace(skip=np.ones_like(lay.skip))               # every env a reset row at every step
    if packed:
        lay.done[:, :, 0] |= 2
    mem = _upload(lay)
    per, parent = _pern(mem, n_step=3, gamma=0.99, beta=0.4), _per(mem, beta=0.4)
    u = torch.rand(130, device=DEV)
    got = per.sample_from_uniforms(u, with_flags=True, with_length=True)
    want = parent.sample_from_uniforms(u, with_flags=True)
    torch.cuda.synchronize()
    assert per.record()["total"] == 0 and bool((got[6] == -1).all()) and bool((got[5] == 0).all()) and bool((got[9] == 0).all())
    for x, w in zip(got, want):
        assert torch.equal(x.view(torch.uint8), w.view(torch.uint8))
    assert torch.equal(got[0], mem.obs[(9 - 1) % 6, 0, 0].expand(130, 10))          # the parent's documented row
    draw, want = _check_sampler(per, mem, u.cpu().numpy(), _arrays(mem))
    assert (draw.key == -1).all() and not want.live.any()


# ---- 7. a captured sample follows the device count ---------------------------------------------------------------------------------

@pytest.mark.parametrize("packed", [False, True])
def test_captured_sample_follows_the_device_count_across_the_wrap(packed):
    env, mem = _mem(3, packed=packed)
    rows = 193
    per = _pern(mem, n_step=3, gamma=0.99, alpha=1.0, beta=0.4)
    g = torch.Generator(device=DEV).manual_seed(9)
    per.sample(rows, generator=g, with_flags=True, with_length=True)        # the uniforms and every kernel, before the capture
    outs = tuple(torch.empty_like(t) for t in per.sample(rows, generator=g, with_flags=True, with_length=True))
    per.push_count()
    graph = torch.cuda.CUDAGraph()
    graph.register_generator_state(g)
    torch.cuda.synchronize()
    before = _state(per)
    with torch.cuda.graph(graph):
        o = per.sample(rows, generator=g, out=outs, device_count=True)
    assert all(a is b for a, b in zip(o, outs)) and len(o) == 10
    assert np.array_equal(_state(per)[0], before[0])                        # the capture itself ran nothing
    lengths = set()
    for count in range(4, 10):                                              # T = 5: the head passes slot 5 and wraps
        _step(mem, 1)
        assert mem.count == count
        per.push_count()
        torch.cuda.synchronize()
        allocs = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
        graph.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == allocs       # a replay allocates nothing
        # refresh, draw and walk restated at this count, from the state before the replay and the uniforms it drew
        table, rec, draw, want = _expect(per, before, mem, per._u[rows].cpu().numpy(), _arrays(mem))
        before = _state(per)
        assert np.array_equal(before[0], table) and before[1] == rec and rec.seen == count
        _compare(outs, draw, want, per.beta)
        assert want.live.all()
        lengths |= set(want.length.tolist())
    assert {1, 2} <= lengths <= {1, 2, 3}
    other = _pern(mem)
    with pytest.raises(RuntimeError, match="before a graph capture"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            other.sample(77)
    env.close()


# ---- 8. learners -------------------------------------------------------------------------------------------------------------------
LE, LN, LT = 16, 4, 32


@pytest.fixture(scope="module")
def memory():
    from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
    from gym_uav_collision_avoidance_amd.replay import DeviceReplay
    env = BatchedMultiUAVWorld2D(LE, num_agents=LN, device=DEV, seed=3)
    mem = DeviceReplay(env, horizon=LT)
    mem.begin(env.reset())
    g = torch.Generator(device=DEV).manual_seed(103)
    for _ in range(LT + 3):
        mem.action_slot().copy_(torch.rand((LE, LN, 2), generator=g, device=DEV) * 2 - 1)
        mem.step(polar=True, auto_reset="agent0_done", step_cap=12)
    yield mem
    env.close()


def _learner(kind, **kw):
    """The learners at their default widths, the smallest the fused actor and critic kernels take."""
    from gym_uav_collision_avoidance_amd import learners
    cls = {"sac": learners.FusedSAC, "td3": learners.FusedTD3, "ddpg": learners.FusedDDPG}[kind]
    torch.manual_seed(11)                                             # the same initial weights every time
    return cls(device=DEV, generator=torch.Generator(device=DEV).manual_seed(77), **kw)


def _params(agent):
    nets = [getattr(agent, n) for n in ("policy", "actor", "actor_target", "critic", "critic_target") if hasattr(agent, n)]
    return [p.detach().clone() for net in nets for p in net.parameters()]


@pytest.mark.parametrize("kind,per_beta", [("sac", 0.0), ("td3", 0.0), ("ddpg", 0.0), ("sac", 0.4)])
def test_per_n_step_learner_eager_equals_captured_equals_fed(kind, per_beta, memory):
    from gym_uav_collision_avoidance_amd.prioritized_nstep import PrioritizedNStepSampler
    from gym_uav_collision_avoidance_amd.prioritized_replay import PrioritizedReplaySampler
    kw = dict(prioritized=0.6, per_beta=per_beta, memory=memory)
    eager = _learner(kind, per_n_step=3, **kw)
    sampler = eager._sampler
    assert type(sampler) is PrioritizedNStepSampler and sampler.alpha == 0.6 and sampler.beta == per_beta
    assert sampler.n_step == 3 and sampler.gamma == eager._discount() == 0.99
    probe = sampler.sample(256, generator=torch.Generator(device=DEV).manual_seed(1), with_length=True)
    assert set(probe[7].unique().tolist()) == {1, 2, 3} and bool((probe[4] < 1).any() and (probe[4] > 0.97).any())
    first, first_rec = _state(sampler)
    assert set(np.unique(first)) == {0, ONE}                          # the initial fill
    keys, inner = [], sampler.update_priorities

    def spy(key, q, y=None, **kw):
        keys.append((key.clone(), q.clone(), y.clone()))
        return inner(key, q, y, **kw)

    sampler.update_priorities = spy
    for _ in range(6):
        eager.update_parameters(None, 64)
    want_table, want_rec = _state(sampler)
    want_log = eager.losses()
    assert len(keys) == 6 and all(k.shape == (64,) and bool((k >= 0).all()) for k, _, _ in keys)
    # the table moved at the sampled keys, which name the START rows of the walks: within one unit of the restatement fed
    # the recorded keys, q and y in order (the two pow implementations)
    ref_table, ref_rec = first, first_rec
    for key, q, y in keys:
        ref_table, ref_rec = prio_ref.update(ref_table, ref_rec, memory.count, key.cpu().numpy(), q.cpu().numpy(),
                                             y.cpu().numpy().reshape(-1), alpha=0.6, eps=1e-6)
    assert np.abs(want_table.astype(np.int64) - ref_table.astype(np.int64)).max() <= 1
    assert abs(want_rec.p_max - ref_rec.p_max) <= 1 and want_rec.p_max == max(ONE, int(want_table.max()))
    # captured
    graphed = _learner(kind, per_n_step=3, **kw)
    graphed.capture(64)
    assert len(graphed._graphs) == (2 if kind == "td3" else 1) and len(graphed._batch) == 7
    graphed.run(6)
    got_table, got_rec = _state(graphed._sampler)
    got_log = graphed.losses()
    assert got_log.shape == (6, 8) and np.array_equal(got_log.view(np.int32), want_log.view(np.int32))
    assert np.array_equal(got_table, want_table) and got_rec == want_rec
    # a one-step prioritized learner fed the batches of a stand-alone sampler: nothing else in the update changed
    fed = _learner(kind, **kw)
    assert type(fed._sampler) is PrioritizedReplaySampler and fed.per_n_step == 1
    alone = PrioritizedNStepSampler(memory, alpha=0.6, beta=per_beta, n_step=3, gamma=0.99)
    for _ in range(6):
        batch = alone.sample(64, generator=fed.generator)
        fed._sampler.load_state_dict(alone.state_dict())              # the refreshed table: the feedback goes into the
        fed.update_batch(*batch[:5], key=batch[6], weight=batch[5] if per_beta > 0 else None)      # learner's own sampler,
        alone.load_state_dict(fed._sampler.state_dict())              # and comes back for the next draw
    fed_log = fed.losses()
    assert np.array_equal(fed_log.view(np.int32), want_log.view(np.int32))
    assert np.array_equal(_state(fed._sampler)[0], want_table) and _state(fed._sampler)[1] == want_rec
    # and the walk matters: the one-step learner on its own draws differs
    plain = _learner(kind, **kw)
    for _ in range(6):
        plain.update_parameters(None, 64)
    assert not np.array_equal(plain.losses().view(np.int32), want_log.view(np.int32))
    for a in (eager, graphed, fed, plain):
        a.close()


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_per_n_step_one_changes_nothing(kind, memory):
    from gym_uav_collision_avoidance_amd.fused_replay import FusedReplaySampler
    from gym_uav_collision_avoidance_amd.prioritized_replay import PrioritizedReplaySampler
    omitted, one = _learner(kind, prioritized=0.6, memory=memory), _learner(kind, prioritized=0.6, per_n_step=1, memory=memory)
    assert type(omitted._sampler) is type(one._sampler) is PrioritizedReplaySampler
    for agent in (omitted, one):
        for _ in range(6):
            agent.update_parameters(None, 64)
    assert np.array_equal(omitted.losses().view(np.int32), one.losses().view(np.int32))
    assert np.array_equal(_state(omitted._sampler)[0], _state(one._sampler)[0]) and _state(omitted._sampler)[1] == _state(one._sampler)[1]
    assert torch.equal(omitted.generator.get_state(), one.generator.get_state())
    assert all(torch.equal(a, b) for a, b in zip(_params(omitted), _params(one)))
    unprioritized = _learner(kind, per_n_step=1, memory=memory)
    assert type(unprioritized._sampler) is FusedReplaySampler and unprioritized.per_n_step == 1
    for a in (omitted, one, unprioritized):
        a.close()


# ---- 9. the refusals that need a device ------------------------------------------------------------------------------------------------

def test_refusals_on_the_device():
    lay = kl.craft(5, 9, False)
    mem = _upload(lay)
    walk = _walk(mem, 3, 0.99)
    rows = 40
    key = torch.from_numpy(kl.cell_keys(lay)[:rows]).to(DEV)
    good = dict(key=key, reward=torch.zeros(rows, device=DEV), next_state=torch.zeros((rows, 10), device=DEV),
                mask=torch.zeros(rows, device=DEV))
    walk.extend(**good)
    walk.extend(**good, truncated=torch.zeros(rows, dtype=torch.bool, device=DEV), ended=torch.zeros(rows, dtype=torch.uint8, device=DEV),
                length=torch.zeros(rows, dtype=torch.uint8, device=DEV))
    empty = dict(key=key[:0], reward=good["reward"][:0], next_state=good["next_state"][:0], mask=good["mask"][:0])
    walk.extend(**empty)                                               # no rows: nothing is launched
    flag = torch.zeros(rows, dtype=torch.bool, device=DEV)
    bad = [dict(key=key.int()), dict(key=key.cpu()), dict(key=key[:7]), dict(key=key.view(rows, 1)), dict(key=key.tolist()),
           dict(reward=good["reward"].double()), dict(reward=good["reward"].cpu()), dict(reward=torch.zeros((rows, 1), device=DEV)),
           dict(next_state=torch.zeros((rows, 9), device=DEV)), dict(next_state=torch.zeros((10, rows), device=DEV).t()),
           dict(mask=torch.zeros(2 * rows, device=DEV)[::2]), dict(mask=None),
           dict(truncated=flag), dict(ended=flag), dict(truncated=flag, ended=flag.float()), dict(truncated=flag.cpu(), ended=flag),
           dict(length=flag), dict(length=torch.zeros(rows + 1, dtype=torch.uint8, device=DEV))]
    for kw in bad:
        with pytest.raises((ValueError, TypeError), match="uavx: "):
            walk.extend(**{**good, **kw})
    from gym_uav_collision_avoidance_amd.prioritized_nstep import KeyWalk, PrioritizedNStepSampler
    for cls in (KeyWalk, PrioritizedNStepSampler):
        for kw, what in ((dict(n_step=0), "n_step in 1..8"), (dict(n_step=9), "n_step in 1..8"), (dict(n_step=2.5), "n_step in 1..8"),
                         (dict(gamma=1.5), "finite gamma"), (dict(gamma=float("nan")), "finite gamma"), (dict(gamma=-0.1), "finite gamma")):
            with pytest.raises(ValueError, match=f"uavx: {cls.__name__} takes .*{what}"):
                cls(mem, **kw)
    with pytest.raises(ValueError, match=r"alpha in \[0, 1\]"):
        PrioritizedNStepSampler(mem, alpha=2.0)
    # the sampler: everything is refused before the uniforms are drawn
    per = _pern(mem, n_step=3)
    g = torch.Generator(device=DEV).manual_seed(5)
    full = per.sample(64, generator=g, with_flags=True, with_length=True)
    assert [len(per.sample(64, generator=g, out=full[:7] + full[n:])) for n in (10, 9, 7)] == [7, 8, 10]
    assert len(per.sample(64, generator=g, out=full[:9])) == 9
    for kw in (dict(out=full[:5]), dict(out=full + full[:1]), dict(out=full[:9], with_length=True), dict(out=[t.double() for t in full[:7]]),
               dict(out=full[:7] + (full[9].float(),)), dict(out=full[:7] + (full[9][:5],)), dict(out=full[:7] + (full[9].cpu(),))):
        state = g.get_state()
        with pytest.raises(ValueError, match="uavx: out"):
            per.sample(64, generator=g, **kw)
        assert torch.equal(g.get_state(), state)                       # a refused call leaves the generator where it was
    with pytest.raises(ValueError, match="takes 0..1048576 rows"):
        per.sample(2 ** 20 + 1)
    mem.count = 0
    state = g.get_state()
    with pytest.raises(ValueError, match="count == 0"):
        per.sample(8, generator=g)
    with pytest.raises(ValueError, match="count == 0"):
        walk.extend(**good)
    assert torch.equal(g.get_state(), state)

"""FusedAdam(max_grad_norm=...) (libuavx_clip.so, include/uavx_clip.h) on the MI355X: planted gradients whose
norm is a small integer, exactly; random gradients within one float32 ulp of the float64 norm; the coefficient bit for bit
from the norm read back; the step bit for bit the EXISTING FusedAdam step on torch's g * clip_coef (what ties the restated
Adam arithmetic to uavx_optim.hip); non-finite gradients as torch treats them; graph capture with a bound moved between
replays; the learners with and without the keyword; and the calls that are refused before anything is enqueued.

Shapes: test_gpu_optim.py's 16-tensor SIZES table (1 .. 2^22: single elements, tails of 1-3 elements, one block and one
element more, 4097 blocks) with every array aligned, cut one float past a 16-byte boundary (the strided path) and with
.grad alone cut so, and the SAC / DDPG critic shapes of optim_ref."""
import numpy as np
import pytest
import torch

import clip_ref
import optim_ref
from test_gpu_optim import KEYS, SIZES

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIZE_SHAPES = [(n,) for n in SIZES]
BLOCK = 1024


def _api():
    from gym_uav_collision_avoidance_amd import fused_optim
    return fused_optim


def _data(shapes, seed, gscale=1e-2):
    """Seeded float32 p, g, m, v, vmax (above v on about half the elements) and a target, one list per name."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda s: torch.randn(s, generator=g, device=DEV)
    u = lambda s: torch.rand(s, generator=g, device=DEV)
    d = dict(p=[r(s) * 0.1 for s in shapes], g=[r(s) * gscale for s in shapes], m=[r(s) * 0.5 * gscale for s in shapes],
             v=[u(s) * gscale ** 2 for s in shapes], t=[r(s) * 0.1 for s in shapes])
    d["x"] = [v * (0.5 + u(v.shape)) for v in d["v"]]
    return d


def _cut(t, off):
    """A copy of t that starts `off` floats past a 16-byte boundary, inside a flat buffer (off = 0: a plain clone)."""
    if off == 0:
        return t.clone()
    buf = torch.zeros(t.numel() + 8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def _make(d, amsgrad, t0, groups=1, off=0, goff=None, grads=None, lr=3e-4):
    """A torch.optim.Adam over copies of d["p"] in `groups` param groups, d's state at step t0, d["g"] (or `grads`) in
    .grad and copies of the targets; every array cut at `off`, .grad at `goff` (default: off).
    Returns (parameters, optimiser, targets)."""
    goff = off if goff is None else goff
    ps = [torch.nn.Parameter(_cut(p, off)) for p in d["p"]]
    n = len(ps)
    cuts = [ps] if groups == 1 else [ps[:n // 2], ps[n // 2:]]
    opt = torch.optim.Adam([{"params": c} for c in cuts], lr=lr, amsgrad=amsgrad)
    for i, p in enumerate(ps):
        p.grad = _cut((d["g"] if grads is None else grads)[i], goff)
        st = dict(step=torch.tensor(float(t0)), exp_avg=_cut(d["m"][i], off), exp_avg_sq=_cut(d["v"][i], off))
        if amsgrad:
            st["max_exp_avg_sq"] = _cut(d["x"][i], off)
        opt.state[p] = st
    return ps, opt, [_cut(t, off) for t in d["t"]]


def _snap(ps, opt, tgt, fa):
    """Everything a step moves, cloned: parameters, moments, targets and the device step counts."""
    out = [p.detach().clone() for p in ps] + [t.clone() for t in tgt]
    out += [opt.state[p][k].clone() for p in ps for k in KEYS if k in opt.state[p]]
    return out + [fa._steps.clone()]


def _same(a, b):
    """torch.equal with NaNs compared as NaNs."""
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype, i
        assert bool(((x == y) | (x.isnan() & y.isnan())).all()), (i, tuple(x.shape))


def _bits(x):
    return int(np.float32(x).view(np.int32))


def _record(fa):
    """(norm, coef, clipped) of the last step as numpy float32 / int (one host read each: test code)."""
    return np.float32(fa.grad_norm.item()), np.float32(fa.clip_coef.item()), int(fa.clipped_steps.item())


# ---- 1. planted norms --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("off,goff", [(0, 0), (1, 1), (0, 1), (3, 2)], ids=["aligned", "cut1", "grad-cut1", "cut3-grad2"])
def test_planted_norms_are_exact(off, goff):
    d = _data(SIZE_SHAPES, 3)
    zeros = [torch.zeros_like(g) for g in d["g"]]
    ps, opt, tgt = _make(d, False, 0, off=off, goff=goff, grads=zeros)
    fa = _api().FusedAdam(opt, max_grad_norm=1.0)
    grads = [p.grad for p in ps]

    def norm_of(planted):
        for g in grads:
            g.zero_()
        for (i, k), value in planted:
            grads[i][k] = value
        fa.step()
        norm, coef, _ = _record(fa)
        assert _bits(coef) == _bits(clip_ref.coef32(norm, 1.0))
        return float(norm)

    # sixteen 1's, each the LAST element of its tensor (the last of an unaligned tail where numel % 4 != 0): norm 4
    assert norm_of([((i, n - 1), 1.0) for i, n in enumerate(SIZES)]) == 4.0
    # the first element behind a block boundary in every tensor that has one (4 tensors), 12 more first elements: norm 4
    behind = [i for i, n in enumerate(SIZES) if n > BLOCK]
    assert len(behind) == 4
    assert norm_of([((i, BLOCK), 1.0) for i in behind] + [((i, 0), 1.0) for i in range(16) if i not in behind]) == 4.0
    # 3 and 4: norm 5, wherever the 3 lies -- every tensor's first, last and last-but-one element, both sides of every
    # block boundary of the small tensors and of the first, a middle and the last boundary of the 2^22 one
    big = SIZES.index(2 ** 22)
    four = ((big, 2 ** 22 - 1), 4.0)
    places = set()
    for i, n in enumerate(SIZES):
        edges = [0, n - 1, n - 2, n - 3, n - 4, n - 5]
        bounds = range(BLOCK, n, BLOCK) if n < 2 ** 20 else (BLOCK, 2 ** 21, n - BLOCK)
        for b in list(bounds)[:5] + list(bounds)[-1:]:
            edges += [b - 1, b, b + 3, b + 4, b + 255, b + 256]
        places |= {(i, k) for k in edges if 0 <= k < n}
    places.discard(four[0])
    assert len(places) > 100
    for place in sorted(places):
        assert norm_of([(place, 3.0), four]) == 5.0, place
    # and 0: nothing is clipped, nothing is NaN
    assert norm_of([]) == 0.0 and float(fa.clip_coef) == 1.0


# ---- 2., 3. random norms, the coefficient, the count -------------------------------------------------------------------------

@pytest.mark.parametrize("name,shapes,off,goff,gscale", [
    ("sizes", SIZE_SHAPES, 0, 0, 1e-2), ("sizes-cut1", SIZE_SHAPES, 1, 1, 1e-2), ("sizes-grad-cut2", SIZE_SHAPES, 0, 2, 3e2),
    ("sac", optim_ref.SAC_SHAPES, 0, 0, 1e-2), ("ddpg", optim_ref.DDPG_SHAPES, 0, 0, 1e-2), ("sac-big", optim_ref.SAC_SHAPES, 0, 0, 1e18),
    ("ddpg-tiny", optim_ref.DDPG_SHAPES, 0, 0, 1e-20)])
def test_random_norms_coefficient_and_count(name, shapes, off, goff, gscale):
    """grad_norm within ONE float32 ulp of (float32)norm64.  Derived: every product is exact in float64, the float64 sum of
    at most 2^26 terms is within 2^-26 relative of S, far under half a float32 ulp (2^-24), so the device value is the
    correctly rounded norm or its neighbour.  clip_coef is then the float32 restatement on the norm READ BACK, bit for bit,
    and clipped_steps advances exactly when coef < 1."""
    d = _data(shapes, 11, gscale=gscale)
    ps, opt, tgt = _make(d, True, 3, off=off, goff=goff)
    want = np.float32(clip_ref.norm64(d["g"]))
    fa = _api().FusedAdam(opt, target=tgt, max_grad_norm=1.0)
    count = 0
    for bound in (float(want) * 0.5, float(want) * 2.0, float(want), float(np.nextafter(want, np.float32(0))), 1e30, 1e-30):
        if not np.isfinite(np.float32(bound)) or np.float32(bound) == 0:
            continue
        fa.set_max_grad_norm(bound)
        fa.step(update_target=True)
        norm, coef, clipped = _record(fa)
        print(f"{name}: norm {norm!r} (float64 {want!r}), bound {bound!r}, coef {coef!r}")
        assert abs(_bits(norm) - _bits(want)) <= 1, (norm, want)
        expect = clip_ref.coef32(norm, bound)
        assert _bits(coef) == _bits(expect), (coef, expect)
        count += int(expect < 1)
        assert clipped == count
    assert 0 < count < 6
    for p, g in zip(ps, d["g"]):
        assert torch.equal(p.grad.view(torch.int32), g.view(torch.int32))          # .grad is never rewritten


# ---- 4. the step is the existing step on g * coef ----------------------------------------------------------------------------

def _decomposed(d, amsgrad, t0, update_target, groups, off, bound, goff=None):
    """One clipped step, and the UNCLIPPED FusedAdam step on cloned state with .grad = g * clip_coef (torch's float32
    multiply): asserts both leave the same bits everywhere.  Returns the clipped object's record."""
    api = _api()
    ps, opt, tgt = _make(d, amsgrad, t0, groups=groups, off=off, goff=goff)
    fa = api.FusedAdam(opt, target=tgt, max_grad_norm=bound)
    fa.step(update_target=update_target)
    coef = fa.clip_coef.clone()
    qs, opt2, tgt2 = _make(d, amsgrad, t0, groups=groups, off=off, goff=goff)
    for q in qs:
        q.grad = q.grad * coef
    fb = api.FusedAdam(opt2, target=tgt2)
    fb.step(update_target=update_target)
    torch.cuda.synchronize()
    _same(_snap(ps, opt, tgt, fa), _snap(qs, opt2, tgt2, fb))
    assert fa._steps.tolist() == [t0 + 1] * groups
    return _record(fa)


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("update_target", [False, True])
@pytest.mark.parametrize("t0", [0, 999])
def test_step_is_the_existing_step_on_clipped_gradients(t0, update_target, amsgrad):
    d = _data(optim_ref.SAC_SHAPES, 21 + t0 % 7)
    norm = clip_ref.norm64(d["g"])
    _, coef, clipped = _decomposed(d, amsgrad, t0, update_target, 1, 0, norm / 3)
    assert 0.3 < coef < 0.34 and clipped == 1
    # inactive: the unclipped step on g itself
    _, coef, clipped = _decomposed(d, amsgrad, t0, update_target, 1, 0, norm * 2)
    assert coef == 1.0 and clipped == 0
    ps, opt, tgt = _make(d, amsgrad, t0)
    fa = _api().FusedAdam(opt, target=tgt, max_grad_norm=norm * 2)
    fa.step(update_target=update_target)
    qs, opt2, tgt2 = _make(d, amsgrad, t0)
    fb = _api().FusedAdam(opt2, target=tgt2)
    fb.step(update_target=update_target)
    _same(_snap(ps, opt, tgt, fa), _snap(qs, opt2, tgt2, fb))


@pytest.mark.parametrize("name,shapes,off,goff", [("sizes", SIZE_SHAPES, 0, None), ("sizes-cut1", SIZE_SHAPES, 1, None),
                                                  ("sizes-grad-cut3", SIZE_SHAPES, 0, 3), ("ddpg", optim_ref.DDPG_SHAPES, 0, None)])
def test_step_decomposition_on_every_size_and_two_groups(name, shapes, off, goff):
    d = _data(shapes, 31)
    norm = clip_ref.norm64(d["g"])
    one = _decomposed(d, True, 4, True, 1, off, norm / 7, goff)
    # two param groups: ONE norm over both -- the same record as one group over the same tensors (the blocks, and with them
    # the order of the sum, are the same) and not either half's own norm
    two = _decomposed(d, True, 4, True, 2, off, norm / 7, goff)
    assert _bits(one[0]) == _bits(two[0]) and _bits(one[1]) == _bits(two[1])
    half = np.float32(clip_ref.norm64(d["g"][:len(shapes) // 2]))
    assert abs(_bits(two[0]) - _bits(np.float32(norm))) <= 1 < abs(_bits(two[0]) - _bits(half))


# ---- 5. non-finite gradients -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("amsgrad", [False, True])
def test_non_finite_gradients_follow_torch(amsgrad):
    d = _data(optim_ref.DDPG_SHAPES, 41)
    d["g"][2][17, 5] = float("inf")
    norm, coef, clipped = _decomposed(d, amsgrad, 2, True, 1, 0, 1.0)
    assert np.isinf(norm) and norm > 0 and _bits(coef) == _bits(0.0) and clipped == 1          # torch: 1 / (inf + 1e-6)
    d["g"][2][17, 5] = float("-inf")
    norm, coef, clipped = _decomposed(d, amsgrad, 2, True, 1, 0, 1.0)
    assert np.isinf(norm) and norm > 0 and coef == 0.0 and clipped == 1
    d["g"][2][17, 5] = float("nan")
    norm, coef, clipped = _decomposed(d, amsgrad, 2, True, 1, 0, 1.0)
    assert np.isnan(norm) and np.isnan(coef) and clipped == 0                                   # NaN < 1 is false


# ---- 6. capture --------------------------------------------------------------------------------------------------------------

def _eager_run(d, grads, bounds):
    ps, opt, tgt = _make(d, True, 0)
    fa = _api().FusedAdam(opt, target=tgt, max_grad_norm=bounds[0])
    recs = []
    for gs, b in zip(grads, bounds):
        for p, g in zip(ps, gs):
            p.grad.copy_(g)
        fa.set_max_grad_norm(b)
        fa.step(update_target=True)
        for p, g in zip(ps, gs):
            assert torch.equal(p.grad.view(torch.int32), g.view(torch.int32))      # .grad is bit-unchanged by a step
        recs.append(fa._clip_rec.clone())
    torch.cuda.synchronize()
    return _snap(ps, opt, tgt, fa) + recs


def test_graph_replay_equals_eager_steps_and_follows_the_bound():
    K = 4
    api = _api()
    shapes = optim_ref.SAC_SHAPES + [(1027,), (3,)]
    d = _data(shapes, 51)
    g = torch.Generator(device=DEV).manual_seed(52)
    grads = [[torch.randn(s, generator=g, device=DEV) * 1e-2 * (k + 1) for s in shapes] for k in range(K)]
    norm0 = clip_ref.norm64(grads[0])
    bounds = [norm0 / 2, norm0 / 2, norm0 * 100, norm0]           # clipped, clipped harder, not clipped, clipped again
    want = _eager_run(d, grads, bounds)                           # (this also loads the kernels before the capture)
    _same(want, _eager_run(d, grads, bounds))                     # two runs give the same bits
    ps, opt, tgt = _make(d, True, 0)
    fa = api.FusedAdam(opt, target=tgt, max_grad_norm=bounds[0])
    before = _snap(ps, opt, tgt, fa)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fa.step(update_target=True)
    torch.cuda.synchronize()
    _same(_snap(ps, opt, tgt, fa), before)                        # the capture itself ran nothing
    recs, coefs = [], []
    for gs, b in zip(grads, bounds):
        for p, x in zip(ps, gs):
            p.grad.copy_(x)                                       # fresh gradients into the SAME buffers
        fa.set_max_grad_norm(b)                                   # the device slot: the replay follows it
        graph.replay()
        recs.append(fa._clip_rec.clone())
        coefs.append(_record(fa))
    torch.cuda.synchronize()
    _same(_snap(ps, opt, tgt, fa) + recs, want)
    for (norm, coef, _), b in zip(coefs, bounds):
        assert _bits(coef) == _bits(clip_ref.coef32(norm, b))
    assert [c[2] for c in coefs] == [1, 2, 2, 3] and coefs[2][1] == 1.0 and coefs[1][1] < coefs[0][1] < 1.0
    fa.sync_state()
    assert float(opt.state[ps[0]]["step"]) == K


# ---- 7. in the learners ------------------------------------------------------------------------------------------------------

def _learner_tools():
    import test_gpu_learners as tl
    return tl


@pytest.mark.parametrize("kind", ["sac", "ddpg"])
def test_learners_with_an_inactive_bound_equal_the_unclipped_learner(kind):
    tl = _learner_tools()
    batches = tl._random_batches(kind, 256, 3, 61)
    plain, wide = tl._learner(kind), tl._learner(kind, max_grad_norm=1e30)
    for agent in (plain, wide):
        for batch, noise in batches:
            agent.update_batch(*batch, noise=noise)
    torch.cuda.synchronize()
    tl._same(tl._state(wide, kind), tl._state(plain, kind))
    assert np.array_equal(wide.losses().view(np.int32), plain.losses().view(np.int32))
    assert plain.grad_norms() == {"critic": None, "actor": None} and plain.max_grad_norm == (None, None)
    norms = wide.grad_norms()
    for name in ("critic", "actor"):
        norm, coef, clipped = norms[name]
        assert norm.device == DEV and norm.dim() == 0 and clipped.dtype == torch.int64
        assert float(norm) > 0 and float(coef) == 1.0 and int(clipped) == 0
    rows, rep = wide.report()
    assert np.array_equal(rows.view(np.int32), wide.losses().view(np.int32))
    assert rep["critic"] == (float(norms["critic"][0]), 1.0, 0) and rep["actor"] == (float(norms["actor"][0]), 1.0, 0)
    assert plain.report()[1] == {"critic": None, "actor": None}
    for a in (plain, wide):
        a.close()


@pytest.mark.parametrize("kind", ["sac", "ddpg"])
def test_learners_with_a_small_bound_clip_every_step(kind):
    tl = _learner_tools()
    batches = tl._random_batches(kind, 256, 3, 62)
    bound = 1e-3
    agent = tl._learner(kind, max_grad_norm=(bound, None))
    critic_adam, actor_adam = agent._adams()
    assert actor_adam._clip is None and actor_adam.max_grad_norm is None and agent.grad_norms()["actor"] is None
    assert agent.max_grad_norm == (bound, None)
    plain = tl._learner(kind)
    for k, (batch, noise) in enumerate(batches):
        agent.update_batch(*batch, noise=noise)
        norm, coef, clipped = (x.clone() for x in agent.grad_norms()["critic"])
        assert int(clipped) == k + 1 and _bits(coef.item()) == _bits(clip_ref.coef32(np.float32(norm.item()), bound))
        if k == 0:      # from zero state: exp_avg = 0 + (g' − 0)·(1 − β1), g' = grad · coef
            plain.update_batch(*batch, noise=noise)
            for p, q in zip(agent.critic.parameters(), plain.critic.parameters()):
                assert torch.equal(p.grad, q.grad)                 # the same gradient, not rewritten by the clipped step
                b1 = critic_adam.hyper()[1]
                assert torch.equal(critic_adam.optimizer.state[p]["exp_avg"], (p.grad * coef) * (1 - b1))
    assert agent.report()[1]["critic"][2] == 3 == agent.updates
    with pytest.raises(ValueError, match="uavx: set_max_grad_norm needs a .* whose actor optimiser"):
        agent.set_max_grad_norm(1.0)                               # the actor's optimiser was built without clipping
    assert agent.max_grad_norm == (bound, None)
    agent.set_max_grad_norm((0.5, None))
    assert agent.max_grad_norm == (0.5, None) and float(agent._clip_recs[0][4]) == 0.5
    with pytest.raises(ValueError, match="uavx: set_max_grad_norm needs"):
        plain.set_max_grad_norm(1.0)
    for a in (plain, agent):
        a.close()


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
def test_captured_clipped_update_equals_the_eager_one(kind):
    tl = _learner_tools()
    env, memory = tl._memory()
    gen = lambda: torch.Generator(device=DEV).manual_seed(77)
    eager = tl._learner(kind, generator=gen(), max_grad_norm=1e-2)
    for _ in range(3):
        eager.update_parameters(memory, 256)
    torch.cuda.synchronize()
    graphed = tl._learner(kind, generator=gen(), memory=memory, max_grad_norm=1e-2)
    graphed.capture(256)
    graphed.run(3)
    torch.cuda.synchronize()
    tl._same(tl._state(graphed, kind), tl._state(eager, kind))
    assert torch.equal(graphed._ring.view(torch.int32), eager._ring.view(torch.int32))        # losses and both clip records
    assert graphed.report()[1]["critic"][2] == 3
    # a bound moved between replays: the captured update follows it (two replays: TD3's second graph steps the actor)
    graphed.set_max_grad_norm(1e30)
    graphed.run(2)
    assert graphed.report()[1]["critic"][1:] == (1.0, 3) and graphed.report()[1]["actor"][1] == 1.0
    for a in (eager, graphed):
        a.close()
    env.close()


# ---- 8. bad calls ------------------------------------------------------------------------------------------------------------

def test_bad_calls_raise_and_enqueue_nothing():
    api = _api()
    d = _data([(5, 3), (5,)], 81)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), torch.tensor(1.0, device=DEV), torch.tensor(1.0)):
        with pytest.raises(ValueError, match="uavx: max_grad_norm must be a finite float > 0"):
            api.FusedAdam(_make(d, False, 2)[1], max_grad_norm=bad)
    ps, opt, tgt = _make(d, False, 2)
    plain = api.FusedAdam(opt)
    with pytest.raises(ValueError, match="uavx: set_max_grad_norm needs a FusedAdam built with max_grad_norm"):
        plain.set_max_grad_norm(1.0)
    assert not hasattr(plain, "grad_norm")
    with pytest.raises(ValueError, match="uavx: record goes with max_grad_norm"):
        api.FusedAdam(_make(d, False, 2)[1], record=torch.zeros(6, device=DEV))
    with pytest.raises(ValueError, match="uavx: record must be"):
        api.FusedAdam(_make(d, False, 2)[1], max_grad_norm=1.0, record=torch.zeros(5, device=DEV))
    ps, opt, tgt = _make(d, False, 2)
    fa = api.FusedAdam(opt, max_grad_norm=1.0)
    fa.step()
    torch.cuda.synchronize()
    snap, rec = _snap(ps, opt, tgt, fa), fa._clip_rec.clone()
    for bad in (0, -2.0, float("inf"), float("nan"), torch.tensor(1.0, device=DEV), None):
        with pytest.raises(ValueError, match="uavx: max_grad_norm must be a finite float > 0"):
            fa.set_max_grad_norm(bad)
    with pytest.raises(ValueError, match="uavx: .*update_target"):
        fa.step(update_target=True)                                # no target was given
    with pytest.raises(TypeError, match="uavx: refresh"):
        fa.step(refresh=torch.nn.Linear(2, 2))
    keep = ps[1].grad
    ps[1].grad = None
    with pytest.raises(ValueError, match="uavx: .*no .grad"):
        fa.step()
    ps[1].grad = torch.zeros(10, device=DEV)[::2]
    with pytest.raises(ValueError, match="uavx: .grad"):
        fa.step()
    opt.param_groups[0]["lr"] = -1.0                               # refused by the library, before its first launch
    ps[1].grad = keep
    with pytest.raises(RuntimeError, match="uavx: uavx_clip_step failed: invalid argument"):
        fa.step()
    torch.cuda.synchronize()
    _same(_snap(ps, opt, tgt, fa), snap)                           # no rejected call moved anything, the step count included
    assert torch.equal(fa._clip_rec.view(torch.int32), rec.view(torch.int32))
    assert fa.max_grad_norm == 1.0


def test_unclipped_fused_adam_does_not_touch_the_binding(monkeypatch):
    """FusedAdam without max_grad_norm makes the calls it always made: with the binding's load() disabled it still steps."""
    from gym_uav_collision_avoidance_amd import _clip_lib

    def refuse():
        raise AssertionError("libuavx_clip.so was asked for")
    monkeypatch.setattr(_clip_lib, "load", refuse)
    d = _data([(5, 3), (1027,)], 91)
    ps, opt, tgt = _make(d, True, 0)
    fa = _api().FusedAdam(opt, target=tgt, max_grad_norm=None)
    fa.step(update_target=True)
    torch.cuda.synchronize()
    assert fa._clip is None and fa.max_grad_norm is None and not torch.equal(ps[0].detach(), d["p"][0])
    with pytest.raises(AssertionError, match="was asked for"):
        _api().FusedAdam(_make(d, True, 0)[1], max_grad_norm=1.0)

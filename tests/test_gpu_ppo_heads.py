"""PPO's HIP heads (libuavx_ppo.so, ppo_heads.PPOHeads) on the MI355X, kernel level, against the float64
restatement of tests/ppo_heads_ref.py on the same float32 inputs.  Minibatches of B in {1, 63, 64, 65, 255, 256, 257, 1 000,
65 537} rows (the last makes a thread total two partials) gathered without repetition from R = 2B + 3, once without idx.
The criterion for what float32 may cost is test_gpu_ppo.py's: a quantity lies within 4 · e32 of float64, e32 being the
distance (max |Δ| / max |float64|) of the same restatement in float32 on the CPU from float64; for quantities of one element
the largest e32 over eight row orders.  Everything that has to be exact is asserted exactly: Σw, the zeros of rows without
weight and of rows clipped on the pessimistic side, a row's outputs wherever it sits in whatever minibatch, two calls' bytes,
what lies past B and the inputs."""
import functools

import numpy as np
import pytest
import torch

import ppo_heads_ref
import ppo_ref
from ppo_heads_ref import ROW_QUANTITIES, SCALARS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 65537)
COEF = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)
ROW_ORDERS = 8
SENTINEL = 7.0
PAD = 5


@functools.lru_cache(maxsize=None)
def _case(B, identity=False):
    return ppo_heads_ref.make_case(B, seed=100 + B, identity=identity)


@functools.lru_cache(maxsize=None)
def _refs(B, identity=False, ent_coef=COEF["ent_coef"]):
    """(the float64 restatement, the float32 one in eight row orders) of a case."""
    c, coef = _case(B, identity), dict(COEF, ent_coef=ent_coef)
    g = torch.Generator().manual_seed(B)
    orders = [None] + [torch.randperm(B, generator=g) for _ in range(ROW_ORDERS - 1)]
    return (ppo_heads_ref.loss(dtype=torch.float64, **c, **coef),
            [ppo_heads_ref.loss(dtype=torch.float32, order=o, **c, **coef) for o in orders])


@functools.lru_cache(maxsize=None)
def _heads():
    from gym_uav_collision_avoidance_amd.ppo_heads import PPOHeads
    return PPOHeads(DEV)


_BUFFERS = ("_ratio", "_g_mean", "_g_log_std", "_g_v")


def _launch(c, coef=COEF, heads=None):
    """One loss call on device copies of case `c`: CPU clones of what it returned, of the rows past B of every output buffer,
    and whether the inputs are what they were."""
    heads = heads or _heads()
    dev = {k: None if t is None else t.to(DEV) for k, t in c.items()}
    before = {k: None if t is None else t.clone() for k, t in dev.items()}
    B = c["v"].shape[0]
    heads.reserve(B + PAD)
    for name in _BUFFERS:
        getattr(heads, name).fill_(SENTINEL)
    out = heads.loss(**dev, **coef)
    got = {k: getattr(out, k).cpu().clone() for k in out._fields}
    got["past"] = [getattr(heads, name)[B:].cpu().clone() for name in _BUFFERS]
    got["inputs_kept"] = all(t is None or torch.equal(t, before[k]) for k, t in dev.items())
    got["shapes"] = {k: tuple(getattr(out, k).shape) for k in out._fields}
    return got


@functools.lru_cache(maxsize=None)
def _gpu(B, identity=False, ent_coef=COEF["ent_coef"]):
    return _launch(_case(B, identity), dict(COEF, ent_coef=ent_coef))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _against_float64(tag, ref64, ref32, got):
    failed = []
    for q in ROW_QUANTITIES + SCALARS:
        single = ref64[q].numel() == 1
        e32 = max(ppo_ref.distance(r[q], ref64[q]) for r in (ref32 if single else ref32[:1]))
        d = ppo_ref.distance(got[q], ref64[q])
        print(f"{tag} {q:12s} e32 = {e32:.3e}{' (of %d row orders)' % ROW_ORDERS if single else ''}   gpu = {d:.3e}   "
              f"gpu / e32 = {d / e32 if e32 else float('nan'):.2f}")
        if not d <= 4.0 * e32:
            failed.append((q, e32, d))
    assert not failed, failed


def _inputs_reach_the_branches(B, ref64):
    live, ratio, adv = ref64["w"] > 0, ref64["ratio"], ref64["adv"]
    lo, hi = 1.0 - COEF["clip"], 1.0 + COEF["clip"]
    if live.any():
        assert float((ratio[live] - lo).abs().min()) > 1e-3 and float((ratio[live] - hi).abs().min()) > 1e-3
    if B >= 255:
        for sign in (adv > 0, adv < 0):
            for side in (ratio < lo, ratio > hi):
                share = float((live & sign & side).sum()) / float(live.sum())
                assert share >= 0.05, share
        assert 0.15 < 1.0 - float(live.float().mean()) < 0.35 and int((adv == 0).sum()) >= 1


@pytest.mark.parametrize("B", SIZES)
def test_loss_against_the_float64_restatement(B):
    ref64, ref32 = _refs(B)
    _inputs_reach_the_branches(B, ref64)
    assert float(ref64["w"][-1]) == 1.0 and abs(float(ref64["s1"][-1])) > 0.1  # at 65 537 thread 0's second partial is this row
    got = _gpu(B)
    assert got["shapes"] == dict(policy_loss=(), value_loss=(), entropy=(), n=(), ratio=(B,), g_mean=(B, 2), g_log_std=(B, 2),
                                 g_v=(B,))
    assert float(got["n"]) == float(ref64["n"])                              # Σw is exact
    _against_float64(f"B = {B}:", ref64, ref32, got)
    assert all(bool((t == SENTINEL).all()) for t in got["past"]) and got["inputs_kept"]


def test_loss_without_idx_reads_the_first_rows():
    ref64, ref32 = _refs(1000, True)
    _inputs_reach_the_branches(1000, ref64)
    got = _gpu(1000, True)
    assert float(got["n"]) == float(ref64["n"])
    _against_float64("identity:", ref64, ref32, got)
    assert all(bool((t == SENTINEL).all()) for t in got["past"]) and got["inputs_kept"]


def test_rows_without_weight_and_rows_clipped_on_the_pessimistic_side_are_exact_zeros():
    B = 1000
    ref64, got = _refs(B)[0], _gpu(B)
    dead = ref64["w"] == 0
    assert 100 < int(dead.sum()) < 400
    for q in ("g_mean", "g_log_std", "g_v"):
        assert bool((got[q][dead] == 0).all()), q
        assert bool((got[q][~dead] != 0).any()), q
    # without the entropy term a live row whose ratio left the band on the side the minimum keeps has no policy gradient
    ref0, got0 = _refs(B, False, 0.0)[0], _gpu(B, False, 0.0)
    clipped = ~dead & ~ref0["passes"]
    moving = ~dead & ref0["passes"] & (ref0["adv"] != 0)
    assert int(clipped.sum()) >= 0.1 * int((~dead).sum()) and int(moving.sum()) >= 0.3 * int((~dead).sum())
    assert bool((got0["g_mean"][clipped] == 0).all()) and bool((got0["g_log_std"][clipped] == 0).all())
    zero = (got0["g_mean"] == 0).all(-1) & (got0["g_log_std"] == 0).all(-1)
    assert int((zero & ~dead & (ref0["adv"] != 0)).sum()) == int((clipped & (ref0["adv"] != 0)).sum())
    assert not bool((zero & moving).any())
    assert bool((got0["g_v"][~dead] != 0).all())                              # the value term does not know about the clip
    # with it every live row has one
    assert bool((got["g_log_std"][~dead] != 0).any(-1).all())


def test_a_row_computes_the_same_bits_wherever_it_sits():
    """Weights of 0 or 2^-12 keep Σw below 1, so D = 1 in every call and no rescaling hides a difference: the same 1 000 rows
    in another order, and as two halves each followed by 277 rows of weight 0, give the same per-row bits."""
    B, half, pad = 1000, 500, 277
    c = dict(_case(B))
    c["weight"] = c["weight"] * 2.0 ** -12
    full = _launch(c)
    assert 0.0 < float(full["n"]) < 1.0
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(77))
    moved = _launch(dict(c, mean=c["mean"][perm], log_std=c["log_std"][perm], v=c["v"][perm], idx=c["idx"][perm]))
    assert not torch.equal(moved["ratio"], full["ratio"])
    for q in ROW_QUANTITIES:
        assert torch.equal(_bits(moved[q]), _bits(full[q][perm])), q
    unused = torch.ones(c["weight"].shape[0], dtype=torch.bool)
    unused[c["idx"]] = False
    spare = torch.nonzero(unused).reshape(-1)[:pad]
    weight = c["weight"].clone()
    weight[spare] = 0.0
    g = torch.Generator().manual_seed(78)
    for rows in (slice(0, half), slice(half, B)):
        part = dict(c, weight=weight, idx=torch.cat([c["idx"][rows], spare]),
                    mean=torch.cat([c["mean"][rows], torch.randn((pad, 2), generator=g)]),
                    log_std=torch.cat([c["log_std"][rows], torch.zeros((pad, 2))]),
                    v=torch.cat([c["v"][rows], torch.randn(pad, generator=g)]))
        got = _launch(part)
        assert got["shapes"]["ratio"] == (half + pad,) and float(got["n"]) < 1.0
        for q in ROW_QUANTITIES:
            assert torch.equal(_bits(got[q][:half]), _bits(full[q][rows])), q
        for q in ("g_mean", "g_log_std", "g_v"):
            assert bool((got[q][half:] == 0).all()), q


def test_two_calls_give_the_same_bytes_and_a_side_stream_works():
    for B in (257, 65537):
        first, again = _gpu(B), _launch(_case(B))
        for q in ROW_QUANTITIES + SCALARS + ("n",):
            assert torch.equal(_bits(first[q]), _bits(again[q])), (B, q)
    from gym_uav_collision_avoidance_amd.ppo_heads import PPOHeads
    stream = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        side = _launch(_case(1000), heads=PPOHeads(DEV))
    stream.synchronize()
    for q in ROW_QUANTITIES + SCALARS + ("n",):
        assert torch.equal(_bits(side[q]), _bits(_gpu(1000)[q])), q


def test_degenerate_weights():
    B = 257
    c = dict(_case(B))
    none = _launch(dict(c, weight=torch.zeros_like(c["weight"])))
    assert float(none["n"]) == 0.0
    for q in SCALARS + ("g_mean", "g_log_std", "g_v"):
        assert bool((none[q] == 0).all()), q                                 # D = 1: ±0, not 0 / 0
    assert bool(torch.isfinite(none["ratio"]).all()) and torch.equal(_bits(none["ratio"]), _bits(_gpu(B)["ratio"]))
    # exactly one live row, in the second workgroup: the means are that row's terms over D = 1
    b = 256
    j = int(c["idx"][b])
    one = torch.zeros_like(c["weight"])
    one[j] = 1.0
    got = _launch(dict(c, weight=one))
    assert float(got["n"]) == 1.0
    f = lambda x: np.float32(x)
    r, a, dv = f(got["ratio"][b]), f(c["adv"][j]), f(c["v"][b]) - f(c["ret"][j])
    s1, s2 = r * a, np.clip(r, f(1.0 - COEF["clip"]), f(1.0 + COEF["clip"])) * a
    assert a != 0 and f(got["policy_loss"]) == -min(s1, s2) and f(got["value_loss"]) == f(0.5) * (dv * dv)
    want, scale = ppo_ref.log_density(c["mean"][b].double(), c["log_std"][b].double(), c["u"][j].double())
    assert abs(float(got["entropy"]) + float(want)) <= 2.0 ** -19 * float(scale)
    live = torch.zeros(B, dtype=torch.bool)
    live[b] = True
    for q in ("g_mean", "g_log_std", "g_v"):
        assert bool((got[q][~live] == 0).all()) and bool((got[q][live] != 0).any()), q
    assert f(got["g_v"][b]) == f(COEF["vf_coef"]) * dv                       # k = 1


# ---- the sampling head -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sampled(rows):
    """Inputs of the loss cases' kind in a ring-like shape [rows, 1, 2]: what sample() wrote, past sentinels included."""
    g = torch.Generator().manual_seed(200 + rows)
    mean = torch.randn((rows, 1, 2), generator=g)
    log_std = torch.rand((rows, 1, 2), generator=g) * 5.0 - 4.0
    eps = torch.randn((rows, 1, 2), generator=g)
    few = max(1, rows // 50)
    log_std[torch.randperm(rows, generator=g)[:few], 0, 0] = -20.0
    log_std[torch.randperm(rows, generator=g)[:few], 0, 1] = 2.0
    u = torch.full((rows + PAD, 1, 2), SENTINEL, device=DEV)
    action = torch.full((rows + PAD, 1, 2), SENTINEL, device=DEV)
    logp = torch.full((rows + PAD, 1), SENTINEL, device=DEV)
    dev = [t.to(DEV) for t in (mean, log_std, eps)]
    _heads().sample(*dev, u[:rows], logp[:rows], action[:rows])
    kept = all(torch.equal(a.cpu(), b) for a, b in zip(dev, (mean, log_std, eps)))
    return mean, log_std, eps, u.cpu(), logp.cpu(), action.cpu(), kept


@pytest.mark.parametrize("rows", (1, 257, 1000, 65537))
def test_sample_against_float64(rows):
    mean, log_std, eps, u, logp, action, kept = _sampled(rows)
    assert kept and bool((u[rows:] == SENTINEL).all()) and bool((logp[rows:] == SENTINEL).all())
    assert bool((action[rows:] == SENTINEL).all())
    u, logp, action = u[:rows], logp[:rows], action[:rows]
    u64, a64, _ = ppo_heads_ref.sample(mean, log_std, eps, torch.float64)
    if rows >= 257:                                                          # a head that squashed μ would be seen
        assert float(((a64 - torch.tanh(mean.double())).abs() > 1e-2).double().mean()) > 0.5
    sigma = torch.exp(log_std.double())
    err_u = (u.double() - u64).abs()
    assert bool((err_u <= 2.0 ** -20 * (mean.double().abs() + sigma * eps.double().abs())).all())
    err_a = (action.double() - torch.tanh(u.double())).abs()
    assert bool((err_a <= 2.0 ** -20).all()) and float(action.abs().max()) <= 1.0
    want, scale = ppo_ref.log_density(mean.double(), log_std.double(), u.double())
    err = (logp.double() - want).abs()
    print(f"rows = {rows}: worst |u - u64| {float(err_u.max()):.3e}, |a - tanh64(u)| {float(err_a.max()):.3e}, "
          f"|log pi - float64| / (2^-19 sum|terms|) {float((err / (2.0 ** -19 * scale)).max()):.3f}")
    assert bool((err <= 2.0 ** -19 * scale).all())


def test_the_loss_head_sees_ratio_one_on_what_sample_stored():
    rows = 1000
    mean, log_std, eps, u, logp, action, _ = _sampled(rows)
    g = torch.Generator().manual_seed(9)
    flat = lambda t: t[:rows].reshape(rows, *t.shape[2:]).contiguous()
    c = dict(mean=flat(mean), log_std=flat(log_std), v=torch.randn(rows, generator=g), idx=None, u=flat(u), logp_old=flat(logp),
             adv=torch.randn(rows, generator=g), ret=torch.randn(rows, generator=g), weight=torch.ones(rows))
    got = _launch(c)
    assert bool((got["ratio"] == 1.0).all()) and float(got["n"]) == rows

"""FusedActor / FusedCritic / FusedTarget (libuavx_actor.so) at every kind of layer size the C ABI accepts, not only the
reference's (256, 256) and (400, 300): partial 16-unit blocks in layer 1 (hidden1 241 / 248, 385 / 393), layer-2 block
counts from 1 to 256 (fewer layer-2 groups than the small-batch critic has waves), actor and critic of different sizes in
one target launch, non-default learner constants, SAC's log_std clamps, and the bf16 kernels against a float64 emulation
of their exact rounding (tests/fused_ref.py).  f32 bounds are those of test_gpu_actor.py /
test_gpu_critic.py; each test prints its measured worst case (pytest -s)."""
import copy

import pytest
import torch

from fused_ref import actor, critic, emu_heads, emu_q, emu_target, heads, q_module, target_torch
from gym_uav_collision_avoidance_amd import _actor_lib as A

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# (hidden1, hidden2) pairs: every hidden1 meets a hidden2 below 16, one that is no multiple of 32, and 4096
SHAPES = {
    "twin": [(241, 1), (241, 33), (241, 4096), (248, 15), (248, 17), (248, 255), (248, 4096), (256, 16), (256, 31),
             (256, 100), (256, 300), (256, 4096)],
    "ddpg": [(385, 1), (385, 33), (385, 4096), (393, 15), (393, 17), (393, 255), (393, 4096), (400, 16), (400, 31),
             (400, 100), (400, 300), (400, 4096)],
}
CASES = [(k, h1, h2) for k in ("sac", "td3", "ddpg") for h1, h2 in SHAPES["ddpg" if k == "ddpg" else "twin"]]
REF_SHAPE = {"sac": (256, 256), "td3": (256, 256), "ddpg": (400, 300)}
ACTOR_ROWS = (1, 17, 64, 65, 129, 4097)
CRITIC_ROWS = (1, 17, 64, 65, 129, 4097, 16383, 16384, 20000)   # around UAVX_CRITIC_SPLIT_ROWS
SPLITS = (A.SPLIT_ROWS, 0, 1 << 62)                               # default, never small-batch, always small-batch
# the target with actor and critic of different sizes (hidden1 within one register tile)
PAIRS = [("sac", (256, 16), (241, 300)), ("sac", (241, 4096), (248, 17)), ("td3", (248, 1), (256, 4096)),
         ("td3", (256, 300), (241, 33)), ("ddpg", (400, 17), (385, 4096)), ("ddpg", (385, 255), (393, 15))]


def _id(case):
    return "-".join(str(x) if not isinstance(x, tuple) else "x".join(map(str, x)) for x in case)


def _report(test, **vals):
    print(f"\nMEASURED {test}: " + ", ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in vals.items()))


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _obs(rows, seed):
    return torch.randn((rows, 10), generator=_gen(seed), device=DEV)


def _fa(m, precision="f32"):
    from gym_uav_collision_avoidance_amd.fused_actor import FusedActor
    return FusedActor.from_module(m, precision=precision)


def _fc(c, precision="f32"):
    from gym_uav_collision_avoidance_amd.fused_critic import FusedCritic
    return FusedCritic.from_module(c, precision=precision)


def _ft(a, c, precision="f32", **kw):
    from gym_uav_collision_avoidance_amd.fused_critic import FusedTarget
    return FusedTarget(a, c, precision=precision, **kw)


def _fwd(fa, x, mode, eps=None, scale=0.0):
    """One uavx_actor_forward in `mode` (every mode, including SAC's ADD_CLAMP that FusedActor.act does not reach)."""
    cols = 4 if (mode == A.RAW and fa.kind == A.SAC) else 2
    return fa._launch(x, eps, scale, mode, torch.empty((x.shape[0], cols), device=DEV), cols)


def _q(fc, s, a):
    q = fc.q(s, a)
    return torch.cat(q, dim=-1) if isinstance(q, tuple) else q


_REPLAY = {}


def _replay_batch(rows, seed=0):
    """(next_state [B, 10], reward [B], mask [B]) sampled from a DeviceReplay after 160 fused steps of random actions with
    auto-reset, so that masks of 0 occur (test_gpu_critic.py's ring)."""
    if "mem" not in _REPLAY:
        from gym_uav_collision_avoidance_amd import BatchedMultiUAVWorld2D
        from gym_uav_collision_avoidance_amd.replay import DeviceReplay
        env = BatchedMultiUAVWorld2D(1024, num_agents=4, device=DEV, seed=31)
        mem = DeviceReplay(env, horizon=160)
        mem.begin(env.reset())
        g = _gen(5)
        for _ in range(160):
            mem.action_slot().copy_(torch.rand((1024, 4, 2), generator=g, device=DEV) * 2 - 1)
            mem.step(polar=True, auto_reset="agent0_done", step_cap=60)
        _REPLAY.update(env=env, mem=mem)
    _, _, r, s2, m = _REPLAY["mem"].sample(rows, generator=_gen(100 + seed))
    return s2.contiguous(), r.contiguous(), m.contiguous()


def _f32_bounds(e_f, e_t, mag, what):
    """test_gpu_actor.py / test_gpu_critic.py's f32 rule: <= max(3 x torch-f32's own error, 2e-6 x mag) and <= 1e-5 x mag,
    mag = max(1, max|ref|).  (torch-f32 itself stays under 1e-5 x mag at every shape here, hidden2 4096 included: 7e-7.)"""
    assert e_f <= max(3 * e_t, 2e-6 * mag), (what, e_f, e_t, mag)
    assert e_f <= 1e-5 * mag, (what, e_f, e_t, mag)


def _err(got, ref, t32):
    return (got.double() - ref).abs().max().item(), (t32.double() - ref).abs().max().item(), max(1.0, ref.abs().max().item())


# ---------------------------------------------------------------------------------------------------------------- actor
@pytest.mark.parametrize("kind,h1,h2", CASES, ids=[_id(c) for c in CASES])
def test_actor_f32_every_mode_at_odd_sizes(kind, h1, h2):
    """RAW, DETERMINISTIC, SAC_SAMPLE (SAC) and ADD_CLAMP (every kind) against the float64 module with the same ε, each
    mode within the f32 rule at every row count; act(evaluate=False), its noise drawn as the module's act() draws it, meets
    the same rule with the module's act() as torch-f32.  Measured on an MI355X, worst over modes and rows (fused /
    torch-f32): hidden2 <= 300 6.2e-7 / 4.2e-7 (SAC 241x1 act), at most 2.35x torch-f32's; hidden2 4096 1.16e-6 / 4.4e-7
    (DDPG 393x4096 RAW), and SAC 256x4096 RAW 1.02e-6 / 3.1e-7, the one case above 3x torch-f32, inside the 2e-6 floor."""
    m = actor(kind, h1, h2, seed=h1 + 7 * h2)
    fa = _fa(m)
    n = ACTOR_ROWS[-1]
    x = _obs(n, 1)
    eps = torch.randn((n, 2), generator=_gen(2), device=DEV)
    y64, y32 = heads(copy.deepcopy(m).double(), x.double()), heads(m, x)
    ts = 0.35                                                      # ADD_CLAMP scale: clamping reached in many rows
    refs = {A.RAW: (y64, y32), A.DETERMINISTIC: (torch.tanh(y64[:, :2]), torch.tanh(y32[:, :2])),
            A.ADD_CLAMP: ((torch.tanh(y64[:, :2]) + ts * eps.double()).clamp(-1, 1), (torch.tanh(y32[:, :2]) + ts * eps).clamp(-1, 1))}
    if kind == "sac":
        refs[A.SAC_SAMPLE] = tuple(torch.tanh(y[:, :2] + y[:, 2:].exp() * e) for y, e in ((y64, eps.double()), (y32, eps)))
    worst = {}
    for rows in ACTOR_ROWS:
        for mode, (r64, r32) in refs.items():
            got = _fwd(fa, x[:rows], mode, eps[:rows].contiguous(), ts)
            assert got.shape == r64[:rows].shape
            e_f, e_t, mag = _err(got, r64[:rows], r32[:rows])
            _f32_bounds(e_f, e_t, mag, (kind, h1, h2, rows, mode))
            worst[mode] = max(worst.get(mode, (0, 0)), (e_f, e_t))
    assert bool((refs[A.ADD_CLAMP][0].abs() == 1).any())
    # the public act(): noise drawn from a generator exactly as the module's act() draws it (DDPG: given), against the
    # float64 forward with that noise, torch-f32 being the module's own act()
    e9 = torch.randn((n, 2), generator=_gen(9), device=DEV)
    if kind == "ddpg":
        got, t32 = fa.act(x, evaluate=False, noise=ts * e9), m.act(x, evaluate=False, noise=ts * e9)
    else:
        kw = dict(noise_std=ts) if kind == "td3" else {}
        got, t32 = fa.act(x, evaluate=False, generator=_gen(9), **kw), m.act(x, evaluate=False, generator=_gen(9), **kw)
    if kind == "sac":
        r64 = torch.tanh(y64[:, :2] + y64[:, 2:].exp() * e9.double())
    else:
        r64 = (torch.tanh(y64[:, :2]) + ts * e9.double()).clamp(-1, 1)
    e_f, e_t, mag = _err(got, r64, t32)
    _f32_bounds(e_f, e_t, mag, (kind, h1, h2, "act"))
    _report("actor_f32", kind=kind, h1=h1, h2=h2, act=f"{e_f:.2e}/{e_t:.2e}",
            **{f"m{k}": f"{v[0]:.2e}/{v[1]:.2e}" for k, v in worst.items()})


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
@pytest.mark.parametrize("shape", ["ref", "odd", "wide"])
def test_actor_bf16_matches_exact_emulation(kind, shape):
    """bf16 RAW / DETERMINISTIC against the float64 emulation of the kernel's rounding (fused_ref.emu_heads): max error
    <= 2e-3 x mag, 99.9 % of elements <= 1e-4 x mag (mag = max(1, max|ref|)), mean error <= 1e-2 x torch-bf16's mean error
    against float64.  What remains are f32-vs-float64 sums before a rounding that flip a hidden activation by one bf16 ulp.
    Measured on an MI355X, worst over 20 000 rows of every shape: max 7.5e-4, 99.9 % 4.7e-5, mean 1.1e-3 x torch-bf16's.
    Rounding the weights by truncation instead gives 4.2e-3-6.5e-3 / 3.0e-3-3.8e-3 / 1.4-2.5x."""
    h1, h2 = _bf16_shape(kind, shape)
    m = actor(kind, h1, h2, seed=40 + h2)
    fa = _fa(m, "bf16")
    x = _obs(20000, 3)
    emu = emu_heads(m, x)
    y64 = heads(copy.deepcopy(m).double(), x.double())
    tb = heads(copy.deepcopy(m).to(torch.bfloat16), x.to(torch.bfloat16)).double()
    out = {}
    for mode in (A.RAW, A.DETERMINISTIC):
        got = _fwd(fa, x, mode).double()
        ref, r64, rtb = (emu, y64, tb) if mode == A.RAW else (torch.tanh(emu[:, :2]), torch.tanh(y64[:, :2]), torch.tanh(tb[:, :2]))
        out[mode] = _bf16_vs_emulation(got, ref, r64, rtb, (kind, shape, mode))
    _report("actor_bf16", kind=kind, shape=f"{h1}x{h2}", **{f"m{k}": v for k, v in out.items()})


def _bf16_shape(kind, shape):
    """The reference's shape, a partial layer-1 block with 2 layer-2 blocks, and a partial block with 256."""
    if shape == "ref":
        return REF_SHAPE[kind]
    h1 = {"odd": 393, "wide": 385}[shape] if kind == "ddpg" else {"odd": 248, "wide": 241}[shape]
    return h1, {"odd": 17, "wide": 4096}[shape]


def _bf16_vs_emulation(got, emu, r64, rtb, what):
    """The bf16 criteria against the emulation; returns the measured (max/mag, q99.9/mag, mean / torch-bf16 mean)."""
    err = (got - emu).abs()
    mag = max(1.0, emu.abs().max().item())
    mean_tb = (rtb - r64).abs().mean().item()
    q999 = torch.quantile(err.flatten()[:1 << 24].float(), 0.999).item()
    res = (err.max().item() / mag, q999 / mag, err.mean().item() / mean_tb)
    assert res[0] <= 2e-3, (what, res)
    assert res[1] <= 1e-4, (what, res)
    assert res[2] <= 1e-2, (what, res)
    return "/".join(f"{v:.2e}" for v in res)


# --------------------------------------------------------------------------------------------------------------- critic
@pytest.mark.parametrize("kind,h1,h2", CASES, ids=[_id(c) for c in CASES])
def test_critic_q_f32_at_odd_sizes_both_variants(kind, h1, h2):
    """FusedCritic.q with the small-batch variant forced on, forced off and at its default threshold, every row count
    around UAVX_CRITIC_SPLIT_ROWS: the f32 rule against the float64 module (towers with distinct weights and nonzero
    biases).  Measured on an MI355X, worst over variants and rows (fused / torch-f32): hidden2 <= 300 1.0e-6 / 9.4e-7
    (DDPG 385x1), at most 1.36x torch-f32's; hidden2 4096 1.16e-6 / 7.0e-7 (DDPG 400x4096), at most 2.25x."""
    c = critic(kind, h1, h2, seed=h1 + 3 * h2)
    fc = _fc(c)
    n = CRITIC_ROWS[-1]
    g = _gen(4)
    s = torch.randn((n, 10), generator=g, device=DEV)
    a = torch.rand((n, 2), generator=g, device=DEV) * 2 - 1
    q64 = q_module(copy.deepcopy(c).double(), s.double(), a.double())
    q32 = q_module(c, s, a)
    worst = (0.0, 0.0)
    for split in SPLITS:
        fc.set_split_rows(split)
        for rows in CRITIC_ROWS:
            got = _q(fc, s[:rows], a[:rows])
            assert got.shape == q64[:rows].shape
            e_f, e_t, mag = _err(got, q64[:rows], q32[:rows])
            _f32_bounds(e_f, e_t, mag, (kind, h1, h2, split, rows))
            worst = max(worst, (e_f, e_t))
    _report("q_f32", kind=kind, h1=h1, h2=h2, fused=worst[0], torch_f32=worst[1])


@pytest.mark.parametrize("kind", ["sac", "td3", "ddpg"])
@pytest.mark.parametrize("shape", ["ref", "odd", "wide"])
def test_critic_q_bf16_matches_exact_emulation(kind, shape):
    """bf16 q in both variants against fused_ref.emu_q, with test_actor_bf16_matches_exact_emulation's criteria.
    Measured on an MI355X: max 4.7e-4, 99.9 % 2.9e-5, mean 1.2e-3 x torch-bf16's; both variants alike."""
    h1, h2 = _bf16_shape(kind, shape)
    c = critic(kind, h1, h2, seed=50 + h2)
    fc = _fc(c, "bf16")
    g = _gen(5)
    s = torch.randn((20000, 10), generator=g, device=DEV)
    a = torch.rand((20000, 2), generator=g, device=DEV) * 2 - 1
    emu = emu_q(c, s, a)
    q64 = q_module(copy.deepcopy(c).double(), s.double(), a.double())
    tb = q_module(copy.deepcopy(c).to(torch.bfloat16), s.to(torch.bfloat16), a.to(torch.bfloat16)).double()
    out = {}
    for split in (0, 1 << 62):
        fc.set_split_rows(split)
        out[split] = _bf16_vs_emulation(_q(fc, s, a).double(), emu, q64, tb, (kind, shape, split))
    _report("q_bf16", kind=kind, shape=f"{h1}x{h2}", large=out[0], small=out[1 << 62])


# --------------------------------------------------------------------------------------------------------------- target
def _check_target(name, got, ref, t32, what):
    """test_gpu_critic.py's target rule on y, a', logπ and min Q; returns the worst (fused, torch-f32) error of each."""
    worst = {}
    for q, gv, rv, tv in zip(("y", "a", "logpi", "minq"), got, ref, t32):
        e_f, e_t, mag = _err(gv, rv, tv)
        assert e_f <= max(3 * e_t, 2e-6 * mag), (what, q, e_f, e_t)
        if name == "sac" and q in ("y", "logpi"):
            assert e_f <= 1.1 * e_t + 1e-5 * mag, (what, q, e_f, e_t)
        else:
            assert e_f <= 1e-5 * mag, (what, q, e_f, mag)
        worst[q] = (e_f, e_t)
    return worst


def _run_target(ft, s2, r, m, eps, alpha):
    rows = s2.shape[0]
    aux = torch.empty((rows, 4), device=DEV)
    y = ft(s2, r, m, alpha=alpha, noise=eps, aux=aux)
    assert y.shape == (rows, 1)
    return y, aux[:, 0:2], aux[:, 2:3], aux[:, 3:4]


@pytest.mark.parametrize("name,ashape,cshape", PAIRS, ids=[_id(p) for p in PAIRS])
def test_target_f32_actor_and_critic_of_different_sizes(name, ashape, cshape):
    """One target launch whose actor and critic differ in hidden2 (and hidden1 within one register tile): y and the four
    aux columns within test_gpu_critic.py's target rule, in both variants, on replay-ring batches (masks 0 and 1) and one
    batch with fractional masks.  Measured on an MI355X (fused / torch-f32): SAC y 1.03e-4 / 1.03e-4 and logπ 5.2e-4 /
    5.2e-4; every other quantity <= 3.8e-7 and <= 1.75x torch-f32's."""
    act, c = actor(name, *ashape, seed=60), critic(name, *cshape, seed=61)
    ft = _ft(act, c)
    n = CRITIC_ROWS[-1]
    s2, r, m = _replay_batch(n, seed=1)
    assert bool((m == 0).any()) and bool((m == 1).any())
    frac = torch.rand((n,), generator=_gen(6), device=DEV)
    eps = torch.randn((n, 2), generator=_gen(7), device=DEV)
    al = torch.tensor([0.2], device=DEV)
    worst = {}
    for masks in (m, frac):
        ref = target_torch(name, act, c, s2, r, masks, eps, 0.2)
        t32 = target_torch(name, act, c, s2, r, masks, eps, 0.2, dtype=torch.float32)
        for split in (0, 1 << 62):
            ft.set_split_rows(split)
            for rows in (1, 17, 65, 129, 4097, 16384, n):
                got = _run_target(ft, s2[:rows], r[:rows], masks[:rows], eps[:rows].contiguous(), al)
                w = _check_target(name, got, [t[:rows] for t in ref], [t[:rows] for t in t32], (name, split, rows))
                for k, v in w.items():
                    worst[k] = max(worst.get(k, (0, 0)), v)
    _report("target_f32_pair", name=name, actor=ashape, critic=cshape, **{k: f"{v[0]:.2e}/{v[1]:.2e}" for k, v in worst.items()})


@pytest.mark.parametrize("name", ["sac", "td3", "ddpg"])
@pytest.mark.parametrize("shape", ["ref", "pair"])
def test_target_f32_learner_constants(name, shape):
    """gamma 0.9, policy_noise 0.35, noise_clip 0.15 (asymmetric: exchanging noise std and clip, or dropping either, moves
    a' by up to 0.2 in the rows where the clip is active, which is most of them), SAC's alpha 0.37 as a float and as a
    device tensor; test_gpu_critic.py's target rule.  Measured on an MI355X (fused / torch-f32): SAC logπ 1.13e-4 /
    1.13e-4, y 3.8e-5 / 3.8e-5; every other quantity <= 4.1e-7."""
    kw = dict(gamma=0.9, policy_noise=0.35, noise_clip=0.15)
    if shape == "ref":
        act, c = actor(name, *REF_SHAPE[name], seed=70), critic(name, *REF_SHAPE[name], seed=71)
    else:
        _, ashape, cshape = next(p for p in PAIRS if p[0] == name)
        act, c = actor(name, *ashape, seed=72), critic(name, *cshape, seed=73)
    ft = _ft(act, c, **kw)
    s2, r, m = _replay_batch(4097, seed=2)
    eps = torch.randn((4097, 2), generator=_gen(8), device=DEV)
    assert ((eps * 0.35).abs() > 0.15).float().mean().item() > 0.5           # the clip is active in most rows
    ref = target_torch(name, act, c, s2, r, m, eps, 0.37, **kw)
    t32 = target_torch(name, act, c, s2, r, m, eps, 0.37, dtype=torch.float32, **kw)
    worst = {}
    for alpha in (0.37, torch.tensor([0.37], device=DEV)):
        for split in (0, 1 << 62):
            ft.set_split_rows(split)
            w = _check_target(name, _run_target(ft, s2, r, m, eps, alpha), ref, t32, (name, shape, split))
            for k, v in w.items():
                worst[k] = max(worst.get(k, (0, 0)), v)
    _report("target_f32_constants", name=name, shape=shape, **{k: f"{v[0]:.2e}/{v[1]:.2e}" for k, v in worst.items()})


@pytest.mark.parametrize("shape", [(256, 256), (248, 17)])
@pytest.mark.parametrize("bias", [40.0, -40.0])
def test_sac_log_std_clamps(bias, shape):
    """log_std_linear's bias at +40 / -40 drives every row into the clamp: RAW's columns 2:4 are exactly 2 / -20,
    SAC_SAMPLE meets the f32 rule against float64, and the target's logπ and y meet test_gpu_critic.py's SAC rule
    (<= 1.1 x torch-f32's error + 1e-5 x mag; at log_std -20 the f32 sample x_t - mean rounds to 0 or one ulp of the mean
    in torch-f32 and in the kernel alike).  Measured on an MI355X (fused / torch-f32): sample <= 1.5e-7 / 1.3e-7; logπ
    9.15 / 9.15 (log_std -20), 0.110 / 0.110 (log_std 2); a' and min Q <= 1.1e-7."""
    act, c = actor("sac", *shape, seed=80), critic("sac", *shape, seed=81)
    with torch.no_grad():
        act.log_std_linear.bias.fill_(bias)
    fa = _fa(act)
    x = _obs(4097, 10)
    eps = torch.randn((4097, 2), generator=_gen(11), device=DEV)
    raw = _fwd(fa, x, A.RAW)
    want = 2.0 if bias > 0 else -20.0
    assert bool((raw[:, 2:] == want).all()), raw[:, 2:].unique()
    y64, y32 = heads(copy.deepcopy(act).double(), x.double()), heads(act, x)
    r64 = torch.tanh(y64[:, :2] + y64[:, 2:].exp() * eps.double())
    r32 = torch.tanh(y32[:, :2] + y32[:, 2:].exp() * eps)
    e_f, e_t, mag = _err(_fwd(fa, x, A.SAC_SAMPLE, eps), r64, r32)
    _f32_bounds(e_f, e_t, mag, ("sample", bias, shape))
    ft = _ft(act, c)
    s2, r, m = _replay_batch(4097, seed=3)
    ref = target_torch("sac", act, c, s2, r, m, eps, 0.2)
    t32 = target_torch("sac", act, c, s2, r, m, eps, 0.2, dtype=torch.float32)
    worst = {}
    for split in (0, 1 << 62):
        ft.set_split_rows(split)
        w = _check_target("sac", _run_target(ft, s2, r, m, eps, 0.2), ref, t32, (bias, shape, split))
        for k, v in w.items():
            worst[k] = max(worst.get(k, (0, 0)), v)
    _report("sac_clamp", bias=bias, shape=shape, sample=f"{e_f:.2e}/{e_t:.2e}",
            **{k: f"{v[0]:.2e}/{v[1]:.2e}" for k, v in worst.items()})


@pytest.mark.parametrize("name", ["sac", "td3", "ddpg"])
@pytest.mark.parametrize("shape", ["ref", "pair"])
def test_target_bf16_matches_exact_emulation(name, shape):
    """bf16 target in both variants against fused_ref.emu_target (a' rounded to bf16 before the critic, as the kernel
    does): y, a' and min Q with test_actor_bf16_matches_exact_emulation's criteria, torch's bf16 block giving the mean
    scale.  SAC's logπ is left to the f32 tests: near tanh saturation log(1 - a'^2 + 1e-6) turns an f32-vs-float64
    difference of the mean into errors no emulation bound can hold.  Measured on an MI355X: max 2.8e-4, 99.9 % 4.8e-5,
    mean 1.4e-3 x torch-bf16's."""
    if shape == "ref":
        act, c = actor(name, *REF_SHAPE[name], seed=90), critic(name, *REF_SHAPE[name], seed=91)
    else:
        _, ashape, cshape = next(p for p in PAIRS if p[0] == name)
        act, c = actor(name, *ashape, seed=92), critic(name, *cshape, seed=93)
    ft = _ft(act, c, "bf16")
    s2, r, m = _replay_batch(20000, seed=4)
    eps = torch.randn((20000, 2), generator=_gen(12), device=DEV)
    emu = emu_target(name, act, c, s2, r, m, eps, 0.2)
    r64 = target_torch(name, act, c, s2, r, m, eps, 0.2)
    tb = [t.double() for t in target_torch(name, act, c, s2, r, m, eps, 0.2, dtype=torch.bfloat16)]
    out = {}
    for split in (0, 1 << 62):
        ft.set_split_rows(split)
        got = _run_target(ft, s2, r, m, eps, 0.2)
        for i, q in ((0, "y"), (1, "a"), (3, "minq")):
            if name == "sac" and q == "y":
                continue                                          # y carries α·logπ (see above)
            out[f"{q}_{'small' if split else 'large'}"] = _bf16_vs_emulation(got[i].double(), emu[i], r64[i], tb[i], (name, shape, split, q))
    _report("target_bf16", name=name, shape=shape, **out)


# ---------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_odd_size_determinism_and_row_independence(precision):
    """SAC (248, 17), and the target with a (241, 4096) critic: repeated calls are bitwise equal, and within one variant a
    prefix of the rows gives the same bits as the full batch."""
    act, c = actor("sac", 248, 17, seed=100), critic("sac", 248, 17, seed=101)
    fa, fc = _fa(act, precision), _fc(c, precision)
    x = _obs(20000, 13)
    a = torch.rand((20000, 2), generator=_gen(14), device=DEV) * 2 - 1
    full = _fwd(fa, x, A.RAW)
    assert torch.equal(full, _fwd(fa, x, A.RAW))
    for n in (1, 17, 65, 4097):
        assert torch.equal(_fwd(fa, x[:n], A.RAW), full[:n]), n
    for split in (0, 1 << 62):
        fc.set_split_rows(split)
        qf = _q(fc, x, a)
        assert torch.equal(qf, _q(fc, x, a))
        for n in (1, 17, 65, 4097):
            assert torch.equal(_q(fc, x[:n], a[:n]), qf[:n]), (split, n)
    ft = _ft(act, critic("sac", 241, 4096, seed=102), precision)
    s2, r, m = _replay_batch(20000, seed=5)
    eps = torch.randn((20000, 2), generator=_gen(15), device=DEV)
    for split in (0, 1 << 62):
        ft.set_split_rows(split)
        yf = _run_target(ft, s2, r, m, eps, 0.2)
        assert all(torch.equal(u, v) for u, v in zip(yf, _run_target(ft, s2, r, m, eps, 0.2)))
        for n in (1, 17, 65, 4097):
            yn = _run_target(ft, s2[:n], r[:n], m[:n], eps[:n].contiguous(), 0.2)
            assert all(torch.equal(u, v[:n]) for u, v in zip(yn, yf)), (split, n)

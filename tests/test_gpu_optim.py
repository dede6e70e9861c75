"""FusedAdam and soft_update (libuavx_actor.so, include/uavx_optim.h) on the MI355X against the float64 statement of
tests/optim_ref.py and torch's own float32 Adam: one step on every state tensor, 100-step runs, the soft update bit for bit,
every tensor size and alignment with guard elements, determinism, graph capture, state exchanged with torch.optim.Adam
both ways, and the step inside 100 critic updates of the SAC and DDPG learners.

Accuracy rule: the fused result's max-abs error against float64 is at most
max(2 x the error of torch's float32 Adam.step() on the same device and inputs, ULPS ulp of the tensor's largest magnitude).
The floor is for tensors of a few elements, where torch's own error can be zero by chance: p, m and v are each stored in
float32, which alone costs up to half an ulp of the stored value, and the handful of float32 operations behind each adds
about as much again, so 4 ulp bounds what any correctly rounded evaluation of the formulas can lose."""
import copy

import pytest
import torch

import optim_ref
from grad_ref import critic, params

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ULPS = 4
ULP = 2.0 ** -23
SENTINEL = 12345.0
KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")


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


def _optim(d, amsgrad, t0, lr=3e-4, dtype=torch.float32, capturable=False, fresh=False):
    """A torch.optim.Adam over copies of d["p"] in `dtype` with d's state at step t0 (fresh: no state yet) and d["g"] in
    .grad."""
    ps = [torch.nn.Parameter(p.clone().to(dtype)) for p in d["p"]]
    opt = torch.optim.Adam(ps, lr=lr, amsgrad=amsgrad, capturable=capturable)
    for i, p in enumerate(ps):
        p.grad = d["g"][i].clone().to(dtype)
        if fresh:
            continue
        st = dict(step=torch.tensor(float(t0), dtype=torch.float32, device=DEV if capturable else "cpu"),
                  exp_avg=d["m"][i].clone().to(dtype), exp_avg_sq=d["v"][i].clone().to(dtype))
        if amsgrad:
            st["max_exp_avg_sq"] = d["x"][i].clone().to(dtype)
        opt.state[p] = st
    return ps, opt


def _set_grads(ps, gs):
    for p, g in zip(ps, gs):
        p.grad.copy_(g)


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("t0", [0, 1, 9, 999, 10 ** 5])
def test_one_step_every_state_tensor(t0, amsgrad):
    d = _data(optim_ref.SAC_SHAPES, 100 + t0 % 97)
    fp, fo = _optim(d, amsgrad, t0)
    _api().FusedAdam(fo).step()
    tp, to = _optim(d, amsgrad, t0)
    to.step()
    torch.cuda.synchronize()
    worst, where, beyond = 0.0, None, 0.0
    for i in range(len(fp)):
        p0, g, m, v = (d[k][i].double() for k in "pgmv")
        rp, rm, rv, rx = optim_ref.adam_step(p0, g, m, v, d["x"][i].double() if amsgrad else None, t0 + 1)
        cases = [("p - p_old", fp[i].detach().double() - p0, tp[i].detach().double() - p0, rp - p0, rp),
                 ("exp_avg", fo.state[fp[i]]["exp_avg"].double(), to.state[tp[i]]["exp_avg"].double(), rm, rm),
                 ("exp_avg_sq", fo.state[fp[i]]["exp_avg_sq"].double(), to.state[tp[i]]["exp_avg_sq"].double(), rv, rv)]
        if amsgrad:
            cases.append(("max_exp_avg_sq", fo.state[fp[i]]["max_exp_avg_sq"].double(),
                          to.state[tp[i]]["max_exp_avg_sq"].double(), rx, rx))
        for name, f, t, ref, stored in cases:
            ef, et = float((f - ref).abs().max()), float((t - ref).abs().max())
            floor = ULPS * ULP * float(stored.abs().max())
            if et > 0 and ef / et > worst:
                worst, where = ef / et, (name, tuple(fp[i].shape), ef / (ULP * float(stored.abs().max())))
            if ef > floor and et > 0:
                beyond = max(beyond, ef / et)
            assert ef <= max(2 * et, floor), (name, i, tuple(fp[i].shape), ef, et, floor)
    print(f"t0={t0} amsgrad={amsgrad}: worst fused / torch-f32 error ratio {worst:.3f} at {where[:2]} "
          f"(error {where[2]:.2f} ulp of the tensor's maximum); worst among errors above the floor {beyond:.3f}")


def _many(shapes, amsgrad, lr, mode, steps=100, seed=7):
    """`steps` steps of seeded gradients from fresh state: mode 'fused', 'torch32' or 'ref64'.  Returns the parameters
    (float64, flattened)."""
    d = _data(shapes, seed)
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    grads = [[torch.randn(s, generator=g, device=DEV) * 1e-2 * float(torch.rand((), generator=g, device=DEV))
              for s in shapes] for _ in range(steps)]
    if mode == "ref64":
        ps = optim_ref.run([p.double() for p in d["p"]], [[x.double() for x in gs] for gs in grads], amsgrad, lr=lr)[0]
    else:
        ps, opt = _optim(d, amsgrad, 0, lr=lr, fresh=True)
        step = _api().FusedAdam(opt).step if mode == "fused" else opt.step
        for gs in grads:
            _set_grads(ps, gs)
            step()
    torch.cuda.synchronize()
    return torch.cat([p.detach().double().reshape(-1) for p in ps])


@pytest.mark.parametrize("name,shapes,amsgrad,lr", [("sac", optim_ref.SAC_SHAPES, False, 3e-4),
                                                    ("ddpg_critic", optim_ref.DDPG_SHAPES, True, 1e-3),
                                                    ("ddpg_actor", optim_ref.DDPG_SHAPES, True, 1e-4)])
def test_many_steps(name, shapes, amsgrad, lr):
    pf, p32, p64 = (_many(shapes, amsgrad, lr, m) for m in ("fused", "torch32", "ref64"))
    df, d32 = float((pf - p64).norm()), float((p32 - p64).norm())
    print(f"{name}: |fused - f64| = {df:.3e}, |torch32 - f64| = {d32:.3e}, ratio {df / d32:.3f}")
    assert df <= 2 * d32 + 1e-12, (df, d32)


@pytest.mark.parametrize("tau", [5e-3, 1.0, 0.0])
def test_soft_update_is_bit_exact(tau):
    api = _api()
    d = _data(optim_ref.SAC_SHAPES + [(3,), (1027,)], 31)
    # alone, against both spellings of the reference evaluated by torch on the device
    tgt = [t.clone() for t in d["t"]]
    api.soft_update(tgt, d["p"], tau)
    for t_new, t_old, p in zip(tgt, d["t"], d["p"]):
        a = t_old * (1.0 - tau) + p * tau            # sac.py / ddpg.py
        b = tau * p + (1 - tau) * t_old              # td3.py:153
        assert torch.equal(a, b)
        assert torch.equal(t_new, a), float((t_new - a).abs().max())
    # fused with the Adam step: from the NEW parameters
    for amsgrad in (False, True):
        ps, opt = _optim(d, amsgrad, 4)
        tgt = [t.clone() for t in d["t"]]
        fa = api.FusedAdam(opt, target=tgt, tau=tau)
        fa.step(update_target=True)
        for t_new, t_old, p in zip(tgt, d["t"], ps):
            assert torch.equal(t_new, t_old * (1.0 - tau) + p.detach() * tau)
        before = [t.clone() for t in tgt]
        fa.step(update_target=False)
        fa.step()
        torch.cuda.synchronize()
        for t_new, t_old in zip(tgt, before):
            assert torch.equal(t_new.view(torch.int32), t_old.view(torch.int32))


SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 65536 + 1, 2 ** 22, 7, 1023, 1024, 1025, 4099, 31]      # a full 16-tensor table
GUARD = 8


def _placed(src, offs):
    """Copies of the tensors of src inside sentinel-filled buffers, tensor i starting offs[i] floats past a 16-byte boundary
    with GUARD sentinel floats on each side at least.  Returns (views, buffers, data offsets)."""
    views, bufs, starts = [], [], []
    for t, off in zip(src, offs):
        buf = torch.full((t.numel() + 2 * GUARD + 4,), SENTINEL, device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[GUARD + off:GUARD + off + t.numel()]
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 * off
        views.append(v)
        bufs.append(buf)
        starts.append(GUARD + off)
    return views, bufs, starts


def _guards_intact(views, bufs, starts):
    for v, b, s in zip(views, bufs, starts):
        assert bool((b[:s] == SENTINEL).all()) and bool((b[s + v.numel():] == SENTINEL).all()), v.numel()


def _run_placed(d, offs_by_name):
    """One AMSGrad step with target update over d placed at the given offsets; returns the six result lists."""
    placed = {k: _placed(d[k], offs_by_name[k]) for k in "pgmvxt"}
    ps = [torch.nn.Parameter(v) for v in placed["p"][0]]
    opt = torch.optim.Adam(ps, lr=3e-4, amsgrad=True)
    for i, p in enumerate(ps):
        assert p.data_ptr() == placed["p"][0][i].data_ptr()
        p.grad = placed["g"][0][i]
        opt.state[p] = dict(step=torch.tensor(3.0), exp_avg=placed["m"][0][i], exp_avg_sq=placed["v"][0][i],
                            max_exp_avg_sq=placed["x"][0][i])
    _api().FusedAdam(opt, target=placed["t"][0], tau=5e-3).step(update_target=True)
    torch.cuda.synchronize()
    for k in "pgmvxt":
        _guards_intact(*placed[k])
    return {k: [v.clone() for v in placed[k][0]] for k in "pgmvxt"}


def test_shapes_alignment_and_guards():
    shapes = [(n,) for n in SIZES]
    d = _data(shapes, 41)
    n = len(shapes)
    base = _run_placed(d, {k: [0] * n for k in "pgmvxt"})
    # the aligned run computes the formulas on every element of every tensor (tails and the last block included)
    for i in range(n):
        rp, rm, rv, rx = optim_ref.adam_step(d["p"][i].double(), d["g"][i].double(), d["m"][i].double(), d["v"][i].double(),
                                             d["x"][i].double(), 4)
        rt = optim_ref.soft(d["t"][i].double(), rp, 5e-3)
        for k, ref in (("p", rp), ("m", rm), ("v", rv), ("x", rx), ("t", rt)):
            err = float((base[k][i].double() - ref).abs().max())
            assert err <= 16 * ULP * float(ref.abs().max()), (k, SIZES[i], err)
        assert torch.equal(base["g"][i], d["g"][i])
    variants = [{k: [off] * n for k in "pgmvxt"} for off in (1, 2, 3)]
    variants.append({k: [(i + j) % 4 for i in range(n)] for j, k in enumerate("pgmvxt")})      # every array differently
    variants.append({k: [1 if k == "g" else 0] * n for k in "pgmvxt"})                          # only .grad unaligned
    variants.append({k: [3 if k == "t" else 0] * n for k in "pgmvxt"})                          # only the target
    for offs in variants:
        out = _run_placed(d, offs)
        for k in "pgmvxt":
            for i in range(n):
                assert torch.equal(out[k][i].view(torch.int32), base[k][i].view(torch.int32)), (k, SIZES[i], offs[k][i])
    # the soft update alone
    for off in (0, 1, 2, 3):
        tv, tb, ts = _placed(d["t"], [off] * n)
        sv, sb, ss = _placed(d["p"], [(off + i) % 4 for i in range(n)])
        _api().soft_update(tv, sv, 5e-3)
        torch.cuda.synchronize()
        _guards_intact(tv, tb, ts)
        _guards_intact(sv, sb, ss)
        for i in range(n):
            assert torch.equal(tv[i], d["t"][i] * (1.0 - 5e-3) + d["p"][i] * 5e-3), (SIZES[i], off)
            assert torch.equal(sv[i], d["p"][i])


def test_determinism():
    d = _data(optim_ref.SAC_SHAPES, 51)
    outs = []
    for _ in range(2):
        ps, opt = _optim(d, True, 11)
        tgt = [t.clone() for t in d["t"]]
        fa = _api().FusedAdam(opt, target=tgt)
        for _ in range(3):
            fa.step(update_target=True)
        torch.cuda.synchronize()
        outs.append([p.detach().clone() for p in ps] + tgt + [opt.state[p][k].clone() for p in ps for k in KEYS])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("capturable", [False, True])
def test_graph_replay_equals_eager_steps(capturable):
    K = 5
    api = _api()
    d = _data(optim_ref.SAC_SHAPES, 61)
    wp, wopt = _optim(d, True, 0, fresh=True)                    # a throw-away optimiser loads the kernels before the capture
    api.FusedAdam(wopt, target=[t.clone() for t in d["t"]]).step(update_target=True)
    ep, eopt = _optim(d, True, 0, fresh=True, capturable=capturable)
    et = [t.clone() for t in d["t"]]
    ea = api.FusedAdam(eopt, target=et)
    for _ in range(K):
        ea.step(update_target=True)
    gp, gopt = _optim(d, True, 0, fresh=True, capturable=capturable)
    gt = [t.clone() for t in d["t"]]
    ga = api.FusedAdam(gopt, target=gt)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ga.step(update_target=True)
    for p, q in zip(gp, d["p"]):
        assert torch.equal(p.detach(), q)                          # the capture itself ran nothing
    for _ in range(K):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(gp + gt, ep + et):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
    for p, q in zip(gp, ep):
        for k in KEYS:
            assert torch.equal(gopt.state[p][k], eopt.state[q][k]), k
    # the count comes back in torch's own layout: what a torch.optim.Adam of the same flags holds after K steps
    tp, topt = _optim(d, True, 0, fresh=True, capturable=capturable)
    for _ in range(K):
        topt.step()
    for a in (ga, ea):
        a.sync_state()
    for p, q, r in zip(gp, ep, tp):
        want = topt.state[r]["step"]
        for got in (gopt.state[p]["step"], eopt.state[q]["step"]):
            assert got.dtype == want.dtype and got.device == want.device and got.shape == want.shape
            assert float(got) == float(want) == K
    assert set(ga.state_dict()["state"][0]) == set(topt.state_dict()["state"][0])


def _flat(ps):
    return torch.cat([p.detach().double().reshape(-1) for p in ps])


def test_state_is_exchanged_with_torch_both_ways():
    k1, k2 = 7, 13
    shapes = optim_ref.DDPG_SHAPES
    d = _data(shapes, 71)
    g = torch.Generator(device=DEV).manual_seed(72)
    grads = [[torch.randn(s, generator=g, device=DEV) * 1e-2 for s in shapes] for _ in range(k1 + k2)]
    p64 = torch.cat([p.reshape(-1) for p in optim_ref.run([p.double() for p in d["p"]],
                                                          [[x.double() for x in gs] for gs in grads], True, lr=1e-3)[0]])

    def run(first, second, hand_over):
        ps, opt = _optim(d, True, 0, lr=1e-3, fresh=True)
        stepper = first(opt)
        for gs in grads[:k1]:
            _set_grads(ps, gs)
            stepper.step()
        ps, opt = hand_over(ps, opt, stepper)
        stepper = second(opt)
        for gs in grads[k1:]:
            _set_grads(ps, gs)
            stepper.step()
        if hasattr(stepper, "sync_state"):
            stepper.sync_state()
        torch.cuda.synchronize()
        steps = [float(opt.state[p]["step"]) for p in ps]
        assert steps == [float(k1 + k2)] * len(ps), steps
        return _flat(ps)

    def fresh_torch(ps, opt, stepper):
        """state_dict() of the wrapper into a new torch.optim.Adam over copies of the parameters."""
        qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        for q in qs:
            q.grad = torch.zeros_like(q)
        new = torch.optim.Adam(qs, lr=1e-3, amsgrad=True)
        sd = stepper.state_dict()
        assert float(sd["state"][0]["step"]) == k1
        new.load_state_dict(sd)
        return qs, new

    keep = lambda ps, opt, stepper: (ps, opt)
    FA = _api().FusedAdam
    p32 = run(lambda o: o, lambda o: o, keep)
    pa = run(lambda o: o, FA, keep)                       # (a) torch steps, then FusedAdam on that optimiser
    pb = run(FA, lambda o: o, fresh_torch)                # (b) fused steps, state_dict() into a fresh torch optimiser
    d32 = float((p32 - p64).norm())
    for name, p in (("torch->fused", pa), ("fused->torch", pb)):
        df = float((p - p64).norm())
        print(f"{name}: |x - f64| = {df:.3e}, |torch32 - f64| = {d32:.3e}, ratio {df / d32:.3f}")
        assert df <= 2 * d32 + 1e-12, (name, df, d32)
    # a reference checkpoint loaded through the wrapper continues at its step
    ps, opt = _optim(d, True, 0, lr=1e-3, fresh=True)
    for gs in grads[:k1]:
        _set_grads(ps, gs)
        opt.step()
    qs, opt2 = _optim(d, True, 0, lr=1e-3, fresh=True)
    fa = FA(opt2)
    fa.load_state_dict(opt.state_dict())
    with torch.no_grad():
        for q, p in zip(qs, ps):
            q.copy_(p)
    for gs in grads[k1:]:
        _set_grads(qs, gs)
        fa.step()
    assert float(fa.state_dict()["state"][0]["step"]) == k1 + k2
    assert float((_flat(qs) - p64).norm()) <= 2 * d32 + 1e-12


def _train(kind, mode, steps=100, rows=256, tau=5e-3):
    """`steps` critic updates of the learner with a soft-updated target critic: y from FusedTarget on the (float32) target in
    every mode, so that the runs differ in the loss gradient, the Adam step and the soft update alone.
    mode 'fused': FusedCriticLoss + FusedAdam.step(update_target=True, refresh=target); 'torch32' / 'torch64': autograd,
    torch's Adam, the reference's soft-update loop and refresh() in that dtype (float64: the target handed to FusedTarget is
    the float64 target rounded to float32)."""
    from gym_uav_collision_avoidance_amd.fused_critic import FusedCriticLoss, FusedTarget
    from gym_uav_collision_avoidance_amd.policy import DDPGActor, GaussianPolicy
    dtype = torch.float64 if mode == "torch64" else torch.float32
    torch.manual_seed(21)
    actor = (GaussianPolicy() if kind == "sac" else DDPGActor()).to(DEV)
    m0 = critic(kind, 22, device=DEV)
    t32 = copy.deepcopy(m0)                                  # what FusedTarget packs
    tgt = FusedTarget(actor, t32)
    m = copy.deepcopy(m0).to(dtype)
    t = t32 if dtype == torch.float32 else copy.deepcopy(m0).to(dtype)
    opt = torch.optim.Adam(m.parameters(), lr=3e-4, amsgrad=kind == "ddpg")
    if mode == "fused":
        cl = FusedCriticLoss(m)
        fa = _api().FusedAdam(opt, target=t, tau=tau)
    g = torch.Generator(device=DEV).manual_seed(23)
    for _ in range(steps):
        s = torch.randn((rows, 10), generator=g, device=DEV)
        a = torch.rand((rows, 2), generator=g, device=DEV) * 2 - 1
        s2 = torch.randn((rows, 10), generator=g, device=DEV)
        r = torch.randn((rows,), generator=g, device=DEV) + 10.0      # keeps q − y off the L1 kink, as §14's run
        mk = (torch.rand((rows,), generator=g, device=DEV) > 0.05).float()
        eps = torch.randn((rows, 2), generator=g, device=DEV)
        y = tgt(s2, r, mk, alpha=0.2, noise=eps if kind == "sac" else None).reshape(-1)
        if mode == "fused":
            cl.backward(s, a, y)
            fa.step(update_target=True, refresh=tgt)
            continue
        opt.zero_grad()
        out = m(s.to(dtype), a.to(dtype))
        qs = list(out) if isinstance(out, tuple) else [out]
        yy = y.to(dtype).reshape(-1, 1)
        loss = sum(torch.nn.functional.mse_loss(q, yy) for q in qs) if kind == "sac" else \
            torch.nn.functional.l1_loss(yy, qs[0])
        loss.backward()
        opt.step()
        with torch.no_grad():
            for tp, p in zip(t.parameters(), m.parameters()):
                tp.data.copy_(tp.data * (1.0 - tau) + p.data * tau)
            if t is not t32:
                for p32, tp in zip(t32.parameters(), t.parameters()):
                    p32.copy_(tp)
        tgt.refresh()
    torch.cuda.synchronize()
    return _flat(params(m)), _flat(params(t))


@pytest.mark.parametrize("kind", ["sac", "ddpg"])
def test_in_the_learner(kind):
    cf, tf = _train(kind, "fused")
    c32, t32 = _train(kind, "torch32")
    c64, t64 = _train(kind, "torch64")
    for name, f, a, b in (("critic", cf, c32, c64), ("target", tf, t32, t64)):
        df, d32 = float((f - b).norm()), float((a - b).norm())
        print(f"{kind} {name}: |fused - f64| = {df:.3e}, |torch32 - f64| = {d32:.3e}, ratio {df / d32:.3f}")
        assert df <= 2 * d32 + 1e-12, (name, df, d32)


def test_bad_calls_raise_and_enqueue_nothing():
    api = _api()
    d = _data([(5, 3), (5,)], 81)
    ps, opt = _optim(d, False, 2)
    fa = api.FusedAdam(opt)
    snap = [p.detach().clone() for p in ps]
    with pytest.raises(ValueError, match="uavx: .*update_target"):
        fa.step(update_target=True)                                # no target was given
    with pytest.raises(TypeError, match="uavx: refresh"):
        fa.step(refresh=torch.nn.Linear(2, 2))
    ps[1].grad = None
    with pytest.raises(ValueError, match="uavx: .*no .grad"):
        fa.step()
    ps[1].grad = torch.zeros(10, device=DEV)[::2]
    with pytest.raises(ValueError, match="uavx: .grad"):
        fa.step()
    torch.cuda.synchronize()
    for p, q in zip(ps, snap):
        assert torch.equal(p.detach(), q)
    fa.sync_state()
    assert float(opt.state[ps[0]]["step"]) == 2.0                  # no rejected call advanced the count
    with pytest.raises(ValueError, match="uavx: .*on cpu"):
        api.FusedAdam(_optim(d, False, 0, fresh=True)[1], target=[t.cpu() for t in d["p"]])
    wide = torch.zeros((4, 6), device=DEV)
    with pytest.raises(ValueError, match="uavx: .*contiguous"):
        api.soft_update([wide[:, :3]], [torch.zeros((4, 3), device=DEV)], 5e-3)
    ps2, opt2 = _optim(d, False, 2)
    opt2.state[ps2[1]]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="uavx: .*different steps"):
        api.FusedAdam(opt2)

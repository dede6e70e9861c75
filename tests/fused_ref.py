"""References shared by the fused actor / critic tests (libuavx_actor.so): policy.py modules of any layer sizes the C ABI
accepts, the float64 forwards of the modules and of the learners' target block, and a float64 emulation of the bf16
kernels' numerics.  A plain module, imported like golden_util.py."""
import copy
import ctypes
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from gym_uav_collision_avoidance_amd import policy

ACTORS = {"sac": policy.GaussianPolicy, "td3": policy.TD3Actor, "ddpg": policy.DDPGActor}
CRITICS = {"sac": policy.TwinQ, "td3": policy.TD3TwinQ, "ddpg": policy.DDPGCritic}

# ---- the hidden sizes uavx_actor_create / uavx_critic_create accept (include/uavx_actor.h, include/uavx_critic.h)
# hidden1 within the last 16-unit block of a compiled register tile, for both precisions: bf16 rounds its layer-1 block
# count up to even, which must not widen the range to 225..240 (SAC / TD3) or 401..416 (DDPG)
HIDDEN1_EDGES = {
    "twin": {"ok": (241, 248, 256), "unsupported": (128, 224, 225, 232, 240, 257, 272)},
    "ddpg": {"ok": (385, 393, 400), "unsupported": (256, 384, 401, 408, 416, 417)},
}
HIDDEN2_EDGES = {"ok": (1, 15, 17, 4096), "unsupported": (4097, 8192), "invalid": (0, -1)}


def check_hidden_range(create, destroy, ok, invalid, unsupported, err_hip):
    """create(kind, prec, 10, h1, h2, 2, &h) at every edge of the documented range, for every kind and precision: inside,
    the call passes validation (OK with a device, where the handle is destroyed again; ERR_HIP from the allocation without
    one); outside, ERR_UNSUPPORTED; hidden2 <= 0 is ERR_INVALID_ARG.  A failed call leaves the handle NULL."""
    bad = []
    for kind in (0, 1, 2):                                  # SAC, TD3, DDPG
        edges = HIDDEN1_EDGES["ddpg" if kind == 2 else "twin"]
        cases = [(h1, 256, "ok") for h1 in edges["ok"]] + [(h1, 256, "unsupported") for h1 in edges["unsupported"]]
        cases += [(edges["ok"][0], h2, what) for what in ("ok", "unsupported", "invalid") for h2 in HIDDEN2_EDGES[what]]
        for prec in (0, 1):                                 # F32, BF16
            for h1, h2, what in cases:
                h = ctypes.c_void_p()
                rc = create(kind, prec, 10, h1, h2, 2, ctypes.byref(h))
                if rc == ok:
                    assert h.value is not None
                    assert destroy(h) == ok
                else:
                    assert h.value is None, (kind, prec, h1, h2, rc)
                want = {"ok": (ok, err_hip), "unsupported": (unsupported,), "invalid": (invalid,)}[what]
                if rc not in want:
                    bad.append(dict(kind=kind, prec=prec, h1=h1, h2=h2, rc=rc, want=want))
    assert not bad, bad


# ---- modules of given layer sizes
def _finish(m, seed, scale, device):
    """Every bias drawn nonzero (TwinQ initialises its biases to 0), U(±1/sqrt(fan_in)) like nn.Linear's; then x scale."""
    g = torch.Generator().manual_seed(10_000 + seed)
    with torch.no_grad():
        for lin in m.modules():
            if isinstance(lin, nn.Linear):
                b = 1.0 / math.sqrt(lin.in_features)
                lin.bias.copy_((torch.rand(lin.bias.shape, generator=g) * 2 - 1) * b)
        if scale != 1:
            for p in m.parameters():
                p.mul_(scale)
    return m.to(device).eval()


def actor(kind, h1, h2, seed, scale=1, device="cuda"):
    """A policy.py actor with hidden sizes (h1, h2): DDPG through its constructor; SAC / TD3 built at hidden=h1 with the
    layers after the first replaced by nn.Linear of the right shapes (their forward uses them by name)."""
    torch.manual_seed(seed)
    if kind == "ddpg":
        m = policy.DDPGActor(hidden1=h1, hidden2=h2)
    elif kind == "sac":
        m = policy.GaussianPolicy(hidden=h1)
        m.linear2, m.mean_linear, m.log_std_linear = nn.Linear(h1, h2), nn.Linear(h2, 2), nn.Linear(h2, 2)
    else:
        m = policy.TD3Actor(hidden=h1)
        m.l2, m.l3 = nn.Linear(h1, h2), nn.Linear(h2, 2)
    return _finish(m, seed, scale, device)


def critic(kind, h1, h2, seed, scale=1, device="cuda"):
    """A policy.py critic with hidden sizes (h1, h2), both towers of a twin critic drawn independently."""
    torch.manual_seed(seed)
    if kind == "ddpg":
        m = policy.DDPGCritic(hidden1=h1, hidden2=h2)
    elif kind == "sac":
        m = policy.TwinQ(hidden=h1)
        m.linear2, m.linear3, m.linear5, m.linear6 = nn.Linear(h1, h2), nn.Linear(h2, 1), nn.Linear(h1, h2), nn.Linear(h2, 1)
    else:
        m = policy.TD3TwinQ(hidden=h1)
        m.l2, m.l3, m.l5, m.l6 = nn.Linear(h1, h2), nn.Linear(h2, 1), nn.Linear(h1, h2), nn.Linear(h2, 1)
    return _finish(m, seed, scale, device)


# ---- the modules' own forwards in their dtype (float64 after .double())
def heads(m, x):
    """Pre-tanh outputs in the module's own dtype: SAC [mean, clamped log_std] (4 columns), TD3 / DDPG 2 columns."""
    with torch.no_grad():
        if isinstance(m, policy.GaussianPolicy):
            return torch.cat(m(x), dim=-1)
        if isinstance(m, policy.TD3Actor):
            return m.l3(F.relu(m.l2(F.relu(m.l1(x)))))
        return m.fc2(F.leaky_relu(m.fc1(F.leaky_relu(m.input(x)))))


def q_module(c, s, a):
    with torch.no_grad():
        q = c(s, a)
    return torch.cat(q, dim=-1) if isinstance(q, tuple) else q


def _target_block(name, pi, qf, s2, r, m, eps, alpha, gamma, policy_noise, noise_clip):
    """The learners' no-grad block with the actor pi (SAC: (mean, log_std); else the tanh action) and critic qf(s, a)."""
    lp = torch.zeros_like(r)
    if name == "sac":                                  # model.py:88-101, sac.py:57-60
        mean, log_std = pi(s2)
        std = log_std.exp()
        normal = torch.distributions.Normal(mean, std, validate_args=False)
        x_t = mean + eps * std
        y_t = torch.tanh(x_t)
        lp = (normal.log_prob(x_t) - torch.log(1 * (1 - y_t.pow(2)) + 1e-6)).sum(1, keepdim=True)
        q1, q2 = qf(s2, y_t)
        mn = torch.min(q1, q2)
        return r + m * gamma * (mn - alpha * lp), y_t, lp, mn
    if name == "td3":                                  # td3.py:116-127
        noise = (eps * policy_noise).clamp(-noise_clip, noise_clip)
        a = (pi(s2) + noise).clamp(-1, 1)
        q1, q2 = qf(s2, a)
        mn = torch.min(q1, q2)
        return r + m * gamma * mn, a, lp, mn
    a = pi(s2)                                         # ddpg.py:62
    q = qf(s2, a)
    return r + gamma * m * q, a, lp, q


def target_torch(name, actor, critic, s2, r, m, eps, alpha, gamma=0.99, dtype=torch.float64, policy_noise=0.2,
                 noise_clip=0.5):
    """The learners' no-grad block in `dtype`: (y [B,1], a' [B,2], logπ [B,1], min Q [B,1])."""
    A, C = copy.deepcopy(actor).to(dtype), copy.deepcopy(critic).to(dtype)
    s2, eps = s2.to(dtype), eps.to(dtype)
    r, m = r.reshape(-1, 1).to(dtype), m.reshape(-1, 1).to(dtype)
    with torch.no_grad():
        return _target_block(name, A, C, s2, r, m, eps, alpha, gamma, policy_noise, noise_clip)


# ---- float64 emulation of the bf16 kernels: observations, weights and the critic's action columns
# rounded to bf16 (round to nearest even); each layer in float64 plus the float32 bias; each hidden activation rounded to
# bf16 after its activation function; the output layer and the epilogue unrounded
def r16(t):
    """float -> bf16 (round to nearest even) -> float64."""
    return t.to(torch.bfloat16).double()


def _layers(m):
    """(hidden layers, output layers, leaky) of an actor, or a list of towers (hidden layers, output layer, leaky)."""
    if isinstance(m, policy.GaussianPolicy):
        return (m.linear1, m.linear2), (m.mean_linear, m.log_std_linear), False
    if isinstance(m, policy.TD3Actor):
        return (m.l1, m.l2), (m.l3,), False
    if isinstance(m, policy.DDPGActor):
        return (m.input, m.fc1), (m.fc2,), True
    if isinstance(m, policy.TwinQ):
        return [((m.linear1, m.linear2), m.linear3, False), ((m.linear4, m.linear5), m.linear6, False)]
    if isinstance(m, policy.TD3TwinQ):
        return [((m.l1, m.l2), m.l3, False), ((m.l4, m.l5), m.l6, False)]
    return [((m.input, m.fc1), m.fc2, True)]


def _emu_hidden(x16, hidden, leaky):
    h = x16
    for lin in hidden:
        z = h @ r16(lin.weight.detach()).T + lin.bias.detach().double()
        h = r16(F.leaky_relu(z) if leaky else F.relu(z))
    return h


def _emu_out(h, lin):
    return h @ r16(lin.weight.detach()).T + lin.bias.detach().double()


@torch.no_grad()
def emu_heads(m, x):
    """The bf16 kernel's pre-tanh outputs of actor m on float32 observations x, in float64 (SAC: 4 columns, log_std
    clamped)."""
    hidden, outs, leaky = _layers(m)
    h = _emu_hidden(r16(x), hidden, leaky)
    y = [_emu_out(h, lin) for lin in outs]
    if len(y) == 2:
        y[1] = y[1].clamp(policy.LOG_SIG_MIN, policy.LOG_SIG_MAX)
    return torch.cat(y, dim=-1)


@torch.no_grad()
def emu_q(c, s, a):
    """The bf16 kernel's Q of critic c on float32 states s and actions a (rounded to bf16 as the kernel does), in float64:
    [B, towers]."""
    x = r16(torch.cat([s, a], dim=-1))
    return torch.cat([_emu_out(_emu_hidden(x, hidden, leaky), out) for hidden, out, leaky in _layers(c)], dim=-1)


@torch.no_grad()
def emu_target(name, actor, critic, s2, r, m, eps, alpha, gamma=0.99, policy_noise=0.2, noise_clip=0.5):
    """The bf16 target kernel in float64: the learners' block on emu_heads, with a' rounded to bf16 before the critic
    (the reported a' is the unrounded one).  Returns (y, a', logπ, min Q) like target_torch."""
    def pi(s):
        y = emu_heads(actor, s)
        return (y[:, :2], y[:, 2:]) if name == "sac" else torch.tanh(y)

    def qf(s, a):
        q = emu_q(critic, s, a)                        # a' (float64) rounded to bf16 inside
        return (q[:, 0:1], q[:, 1:2]) if q.shape[1] == 2 else q

    r, m = r.reshape(-1, 1).double(), m.reshape(-1, 1).double()
    return _target_block(name, pi, qf, s2, r, m, eps.double(), alpha, gamma, policy_noise, noise_clip)

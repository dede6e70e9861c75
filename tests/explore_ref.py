"""The exploration launch (include/uavx_explore.h) restated in float64 numpy: the maps from Philox words to
normals and uniform actions, the order of the per-row decisions, and the three action formulas.  The GPU tests compare the
kernel with these functions and the host tests compare them with the reference's Ornstein-Uhlenbeck class through the
fixture tests/golden/ou_reference.npz (tests/golden/make_explore_golden.py writes it)."""
import json
import os

import numpy as np

from reset_layouts import philox4x32_10

SAC, TD3, DDPG = 0, 1, 2
TWO_PI = 6.283185307179586
INV32 = 1.0 / 4294967296.0
MAX_NORMAL = 6.67               # sqrt(-2 log 2^-32) = 6.6604: no draw is larger
OU_CASES = ((0, 0.2), (7, 0.2), (3, 1.5))       # (np.random.seed, std_deviation) of the fixture's cases
OU_STEPS = 512
OU_THETA, OU_DT, OU_MEAN = 0.15, 1e-2, 0.0      # ou.py's defaults and ddpg.py:31's mean


def words(seed, g, n, stream):
    """The four Philox words of global row(s) g at call count(s) n: key (seed lo, seed hi), counter (g lo, g hi, n, stream)."""
    g = np.asarray(g, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10(g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), np.asarray(n, dtype=np.uint64), stream,
                         seed & 0xFFFFFFFF, seed >> 32)


def normals(w0, w1):
    """Box-Muller in float64 from two words: u1 = (w0 + 1) 2^-32 in (0, 1], u2 = w1 2^-32 in [0, 1)."""
    u1 = (w0.astype(np.float64) + 1.0) * INV32
    u2 = w1.astype(np.float64) * INV32
    r = np.sqrt(-2.0 * np.log(u1))
    t = TWO_PI * u2
    return r * np.cos(t), r * np.sin(t)


def uniform_action(w):
    """np.random.uniform(-1, 1) from a 32-bit word, rounded to float32 once."""
    return (-1.0 + 2.0 * (w.astype(np.float64) * INV32)).astype(np.float32)


def bernoulli_u(w0):
    return w0.astype(np.float64) * INV32


def ou_step(x, n0, sigma, theta=OU_THETA, dt=OU_DT, mean=OU_MEAN):
    """ou.py:18-22 left to right in float64; s = sigma·sqrt(dt) is one product formed first (python's precedence)."""
    s = sigma * np.sqrt(dt)
    return (x + (theta * (mean - x)) * dt) + s * n0


def ou_run(normals0, sigma, x0=0.0, **kw):
    x, out = np.float64(x0), np.empty(len(normals0), dtype=np.float64)
    for k, z in enumerate(normals0):
        x = ou_step(x, np.float64(z), sigma, **kw)
        out[k] = x
    return out


def decide(seed, g, n, warmup_steps, p):
    """Which rows act at random: n < warmup_steps, or p > 0 and the stream-1 uniform below float64(float32(p))."""
    n = np.asarray(n, dtype=np.uint64)
    p = np.float32(p)
    rnd = n < np.uint64(warmup_steps)
    if p > 0:
        rnd = rnd | (bernoulli_u(words(seed, g, n, 1)[0]) < np.float64(p))
    return rnd


def act(kind, raw, x, n, seed, row_offset=0, warmup_steps=0, p=0.0, noise_std=0.1, sigma=0.2, theta=OU_THETA, dt=OU_DT,
        mean=OU_MEAN, x_initial=0.0, fed=None, reset=None, tanh32=None):
    """One call over all rows.  raw: float32 [rows, 4 | 2]; x: float64 [rows]; n: uint32 [rows]; fed: float64 [rows, 2] or
    None; reset: bool [rows] or None.  tanh32: float32 tanh(raw[:, :2]) as the device computed it (the DETERMINISTIC
    launch) for the kinds whose formula starts from it; None takes numpy's.
    Returns (action float64 [rows, 2] BEFORE the rounding to float32 except on random rows, which are exact float32 values;
    x', n', random [rows], the normals used [rows, 2])."""
    rows = raw.shape[0]
    g = (np.arange(rows, dtype=np.uint64) + np.uint64(row_offset))
    w = words(seed, g, n, 0)
    nz = np.stack(normals(w[0], w[1]), axis=1) if fed is None else np.asarray(fed, dtype=np.float64)
    x = np.array(x, dtype=np.float64)
    if reset is not None:
        x[np.asarray(reset, dtype=bool)] = x_initial
    rnd = decide(seed, g, n, warmup_steps, p)
    uni = np.stack([uniform_action(w[2]), uniform_action(w[3])], axis=1).astype(np.float64)
    y = raw.astype(np.float64)
    th = np.tanh(y[:, :2]) if tanh32 is None else tanh32.astype(np.float64)
    z32 = nz.astype(np.float32).astype(np.float64)
    if kind == SAC:
        a = np.tanh(y[:, :2] + np.exp(y[:, 2:4]) * z32)
    elif kind == TD3:
        a = np.clip(th + float(np.float32(noise_std)) * z32, -1.0, 1.0)
    else:
        x2 = ou_step(x, nz[:, 0], sigma, theta, dt, mean)
        x = np.where(rnd, x, x2)
        a = np.clip(th + x[:, None], -1.0, 1.0)
    a = np.where(rnd[:, None], uni, a)
    n2 = ((np.asarray(n, dtype=np.uint64) + np.uint64(1)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return a, x, n2, rnd, nz


def load_fixture(golden_dir):
    """(meta dict, {name: array}) of tests/golden/ou_reference.npz."""
    with np.load(os.path.join(golden_dir, "ou_reference.npz")) as z:
        meta = json.loads(str(z["meta"]))
        return meta, {k: z[k] for k in z.files if k != "meta"}

"""numpy restatement of the replay sampler's semantics (include/uavx_replay.h steps 1-4 and the out-of-range rule), the
reference the GPU tests of FusedReplaySampler compare against.  test_replay_host.py checks it against the torch
expressions of DeviceReplay.sample on CPU tensors."""
import numpy as np


def pick(u, n):
    """trunc(u · (float32)n) clamped into [0, n − 1]: one float32 multiply; NaN and negatives give 0, +inf the top."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = (np.asarray(u, dtype=np.float32) * np.float32(n)).astype(np.float64)
    x = np.where(np.isnan(x), 0.0, x)
    return np.minimum(np.clip(x, 0.0, float(n)).astype(np.int64), n - 1)


def source_rows(valid):
    """src[j]: the largest valid p <= j, without one the smallest valid p > j, without one B − 1."""
    valid = np.asarray(valid, dtype=bool)
    B = valid.shape[0]
    src = np.empty(B, dtype=np.int64)
    last = -1
    for j in range(B):
        if valid[j]:
            last = j
        src[j] = last
    nxt = B - 1
    for j in range(B - 1, -1, -1):
        if valid[j]:
            nxt = j
        if src[j] < 0:
            src[j] = nxt
    return src


def sample(u, obs, act, rew, done, count, T, num_learners, skip=None, trunc=None, ended=None):
    """u [2, 3, B] float32; obs [L, E, N, 10], act [L, E, N, 2], rew [L, E, N] float32, done [L, E, N] uint8; skip, trunc,
    ended [L, E] uint8 or all None (flags in bits 1 / 3 / 2 of done[:, :, 0]); count >= 1 steps written (less is taken as
    1), T = L − 1.  Returns (state, action, reward, next_state, mask, truncated, ended, src)."""
    u = np.asarray(u, dtype=np.float32)
    L, E = obs.shape[0], obs.shape[1]
    assert L == T + 1 and u.shape[:2] == (2, 3)
    count = max(int(count), 1)
    lo = max(0, count - T)
    span = count - lo
    if skip is None:
        skip, trunc, ended = (done[:, :, 0] & 2) != 0, (done[:, :, 0] & 8) != 0, (done[:, :, 0] & 4) != 0
    else:
        skip, trunc, ended = skip != 0, trunc != 0, ended != 0
    k = [lo + pick(u[d, 0], span) for d in (0, 1)]
    e = [pick(u[d, 1], E) for d in (0, 1)]
    i = [pick(u[d, 2], num_learners) for d in (0, 1)]
    bad = skip[k[0] % L, e[0]]
    k, e, i = np.where(bad, k[1], k[0]), np.where(bad, e[1], e[0]), np.where(bad, i[1], i[0])
    valid = ~skip[k % L, e]
    src = source_rows(valid)
    k, e, i = k[src], e[src], i[src]
    s, s1 = k % L, (k + 1) % L
    mask = np.float32(1.0) - (done[s, e, i] & 1).astype(np.float32)
    return obs[s, e, i], act[s, e, i], rew[s, e, i], obs[s1, e, i], mask, trunc[s, e], ended[s, e], src

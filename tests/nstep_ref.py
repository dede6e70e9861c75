"""numpy restatement of the n-step replay sampler's semantics (include/uavx_nstep.h steps 1-4), the reference the GPU tests
of NStepReplaySampler compare against.  Built on replay_ref.pick / source_rows; test_nstep_host.py checks it against a
per-row loop written from the header's prose, against replay_ref.sample for one step, and counts the recency-weighted
draw over an exhaustive grid."""
import collections

import numpy as np

from replay_ref import pick, source_rows

# why a walk ended: every condition of step 3 that held at the last step walked, as bits
N_STEP, DONE, ENDED, HEAD, SKIP = 1, 2, 4, 8, 16
REASONS = {"n_step": N_STEP, "done": DONE, "ended": ENDED, "head": HEAD, "skip": SKIP}

Batch = collections.namedtuple("Batch", "state action reward next_state mask truncated ended src length reason k e i")


def start_rows(u, count, T, envs, num_learners, skip, recency=0.0):
    """Steps 1 and 2: (k, e, i, valid) of every row after the redraw, before the fallback.  u [2, 3 or 5, B] float32,
    skip [L, E] bool."""
    u = np.asarray(u, dtype=np.float32)
    L = T + 1
    cols = u.shape[1]
    assert u.shape[0] == 2 and (cols == 5 or (cols == 3 and recency == 0.0))
    count = max(int(count), 1)
    lo = max(0, count - T)
    span = count - lo
    k = []
    for d in (0, 1):
        ka = pick(u[d, 0], span)
        if cols == 5:
            with np.errstate(invalid="ignore"):
                recent = u[d, 4] < np.float32(recency)          # a NaN compares false
            ka = np.where(recent, np.maximum(ka, pick(u[d, 3], span)), ka)
        k.append(lo + ka)
    e = [pick(u[d, 1], envs) for d in (0, 1)]
    i = [pick(u[d, 2], num_learners) for d in (0, 1)]
    bad = skip[k[0] % L, e[0]]
    k, e, i = np.where(bad, k[1], k[0]), np.where(bad, e[1], e[0]), np.where(bad, i[1], i[0])
    return k, e, i, ~skip[k % L, e]


def sample(u, obs, act, rew, done, count, T, num_learners, n_step, gamma, recency=0.0, skip=None, trunc=None, ended=None):
    """u [2, 3, B] (recency == 0 only) or [2, 5, B] float32; the ring as replay_ref.sample takes it (skip, trunc, ended
    [L, E] uint8, or all None: bits 1 / 3 / 2 of done[:, :, 0]); count >= 1 steps written (less is taken as 1), T = L − 1;
    n_step 1..8, gamma a Python float.  Returns a Batch: the seven outputs, src, length (uint8), reason (the bits above)
    and the (k, e, i) of the start row each row used."""
    L, E = obs.shape[0], obs.shape[1]
    assert L == T + 1 and 1 <= n_step <= 8
    c = max(int(count), 1)
    if skip is None:
        skip, trunc, ended = (done[:, :, 0] & 2) != 0, (done[:, :, 0] & 8) != 0, (done[:, :, 0] & 4) != 0
    else:
        skip, trunc, ended = skip != 0, trunc != 0, ended != 0
    k, e, i, valid = start_rows(u, c, T, E, num_learners, skip, recency)
    src = source_rows(valid)
    k, e, i = k[src], e[src], i[src]
    B = k.shape[0]
    R, g = np.full(B, -0.0, dtype=np.float64), np.ones(B, dtype=np.float64)       # −0 + x is x, for a reward of −0 too
    run = np.ones(B, dtype=bool)
    length, reason = np.zeros(B, dtype=np.uint8), np.zeros(B, dtype=np.int64)
    d_last = np.zeros(B, dtype=np.uint8)
    tr_last, en_last = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    for j in range(n_step):
        kj = np.minimum(k + j, c - 1)                     # rows that have stopped are carried along inside the window
        s = kj % L
        R = np.where(run, R + g * rew[s, e, i].astype(np.float64), R)
        d = done[s, e, i] & 1
        nxt = kj + 1
        why = ((j == n_step - 1) * N_STEP + (d != 0) * DONE + ended[s, e] * ENDED + (nxt >= c) * HEAD
               + ((nxt < c) & skip[nxt % L, e]) * SKIP)
        stop = run & (why != 0)
        d_last, tr_last, en_last = np.where(run, d, d_last), np.where(run, trunc[s, e], tr_last), np.where(run, ended[s, e], en_last)
        length, reason = np.where(stop, j + 1, length).astype(np.uint8), np.where(stop, why, reason)
        run = run & ~stop
        g = np.where(run, g * np.float64(gamma), g)
    assert not run.any()
    s0, sn = k % L, (k + length) % L
    mask = ((1.0 - d_last.astype(np.float64)) * g).astype(np.float32)
    return Batch(obs[s0, e, i], act[s0, e, i], R.astype(np.float32), obs[sn, e, i], mask, tr_last, en_last, src, length,
                 reason, k, e, i)

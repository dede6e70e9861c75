"""numpy restatement of the n-step walk from keys (include/uavx_keywalk.h), written from the header's prose: the reference
the GPU tests of KeyWalk and PrioritizedNStepSampler compare against.  test_keywalk_host.py ties it to nstep_ref.sample,
which test_nstep_host.py proved against a per-row loop: fed the (k, e, i) that restatement reports, this one gives its
batch bit for bit."""
import collections

import numpy as np

from nstep_ref import DONE, ENDED, HEAD, N_STEP, SKIP

Walk = collections.namedtuple("Walk", "reward next_state mask truncated ended length reason live k e i")


def decode(key, count, T, envs, num_learners):
    """-> (live, k, e, i): the step, env and agent a key names, and whether the row is walked (key >= 0 and lo <= k < c).
    k, e, i of a row that is not are 0."""
    key = np.asarray(key, dtype=np.int64)
    c = max(int(count), 1)
    lo = max(0, c - T)
    per = envs * num_learners
    q = np.where(key >= 0, key, 0)
    k, rest = q // per, q % per
    live = (key >= 0) & (k >= lo) & (k < c)
    z = np.zeros_like(q)
    return live, np.where(live, k, z), np.where(live, rest // num_learners, z), np.where(live, rest % num_learners, z)


def walk(key, obs, rew, done, count, T, num_learners, n_step, gamma, skip=None, trunc=None, ended=None):
    """key [B] int64; the ring as nstep_ref.sample takes it (skip, trunc, ended [L, E] uint8, or all None: bits 1 / 3 / 2 of
    done[:, :, 0]); count >= 1 steps written (less is taken as 1), T = L − 1; n_step 1..8, gamma a Python float.  Returns
    a Walk: reward, next_state, mask, truncated, ended (meaningless where not `live`: the kernel leaves those rows alone),
    length (uint8, 0 for an ignored row), reason (the bits of nstep_ref.REASONS, 0 for an ignored row), live, k, e, i."""
    L, E = obs.shape[0], obs.shape[1]
    assert L == T + 1 and 1 <= n_step <= 8
    c = max(int(count), 1)
    if skip is None:
        skip, trunc, ended = (done[:, :, 0] & 2) != 0, (done[:, :, 0] & 8) != 0, (done[:, :, 0] & 4) != 0
    else:
        skip, trunc, ended = np.asarray(skip) != 0, np.asarray(trunc) != 0, np.asarray(ended) != 0
    live, k, e, i = decode(key, c, T, E, num_learners)
    B = k.shape[0]
    R, g = np.full(B, -0.0, dtype=np.float64), np.ones(B, dtype=np.float64)       # −0 + x is x, for a reward of −0 too
    run = live.copy()
    length, reason = np.zeros(B, dtype=np.uint8), np.zeros(B, dtype=np.int64)
    d_last = np.zeros(B, dtype=np.uint8)
    tr_last, en_last = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    for j in range(n_step):
        kj = np.minimum(k + j, c - 1)                     # rows that have stopped are carried along inside the window
        s = kj % L
        with np.errstate(invalid="ignore"):
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
    mask = ((1.0 - d_last.astype(np.float64)) * g).astype(np.float32)
    return Walk(R.astype(np.float32), obs[(k + length) % L, e, i], mask, tr_last, en_last, length, reason, live, k, e, i)

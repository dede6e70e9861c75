"""The running statistics of include/uavx_norm.h restated for the tests.

fold_obs(), fold_returns(), apply_obs() and scale_rewards() are the numpy restatement: float64, vectorised over the columns,
sequential in k, summing in the header's documented order (column sums in walk order k upwards, a halving tree over each 64
columns, four wavefronts left to right, then thread t of one workgroup over partials t, t + 256, ...).  The *_loop functions
are a second writing of the same prose, one column and one Python float at a time, sharing no code with the first.

A record is a dict: n_obs (int), mean and M2 (float64 [F]), n_ret (int), mean_ret and M2_ret (float); new_record(F) is the
empty one.  No function changes its arguments: a fold returns the new record (and the new carry)."""
import math

import numpy as np

BLOCK, WAVE, MAX_FEATURES = 256, 64, 16


def new_record(F):
    return dict(n_obs=0, mean=np.zeros(F), M2=np.zeros(F), n_ret=0, mean_ret=0.0, M2_ret=0.0)


def words(rec):
    """The 36 eight-byte words of uavx_norm_record, as uint64."""
    F = len(rec["mean"])
    w = np.zeros(36, np.float64)
    w[1:1 + F], w[17:17 + F], w[34], w[35] = rec["mean"], rec["M2"], rec["mean_ret"], rec["M2_ret"]
    w = w.view(np.uint64).copy()
    w[0], w[33] = rec["n_obs"], rec["n_ret"]
    return w


def same_words(a, b):
    """Two words() arrays: bit equality, a NaN matching any NaN, in the float64 words; the two counts equal."""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    fa, fb = a.view(np.float64), b.view(np.float64)
    eq = (a == b) | (np.isnan(fa) & np.isnan(fb))
    eq[[0, 33]] = a[[0, 33]] == b[[0, 33]]
    return bool(eq.all())


def _flag_rows(done, skip, ended):
    if (skip is None) != (ended is None):
        raise ValueError("skip and ended come together")
    if skip is None:
        return (done[:, :, 0] & 2) != 0, (done[:, :, 0] & 4) != 0
    return skip != 0, ended != 0


def sample_mask(done, k, learners, skip=None, ended=None):
    """[E, N] bool: which rows of step k are samples."""
    L, E, N = done.shape
    sk, en = _flag_rows(done, skip, ended)
    m = ~sk[k % L][:, None] & (np.arange(N) < learners)[None, :]
    if k >= 1:
        p = (k - 1) % L
        m = m & ~(((done[p] & 1) != 0) & ~sk[p][:, None] & ~en[p][:, None])
    return m


def _reduce(acc):
    """acc [..., columns padded to whole workgroups] of column sums -> [...]: workgroup sums, then the total."""
    lead = acc.shape[:-1]
    w = acc.reshape(lead + (-1, BLOCK // WAVE, WAVE))

    def tree(w):                                  # [..., 4, 64] -> [...]
        off = WAVE // 2
        while off:
            w = w[..., :off] + w[..., off:2 * off]
            off //= 2
        w = w[..., 0]
        r = w[..., 0]
        for j in range(1, BLOCK // WAVE):
            r = r + w[..., j]
        return r

    partial = tree(w)                             # [..., blocks]
    pad = (-partial.shape[-1]) % BLOCK
    partial = np.concatenate([partial, np.zeros(lead + (pad,))], axis=-1).reshape(lead + (-1, BLOCK))
    t = np.zeros(lead + (BLOCK,))
    for j in range(partial.shape[-2]):
        t = t + partial[..., j, :]
    return tree(t.reshape(lead + (1, BLOCK // WAVE, WAVE)))[..., 0]


def _batch(rows, masks):
    """rows: per step, oldest first, [..., columns] float64 samples; masks: per step [columns] bool.  (n_b, mean_b, M2_b)."""
    cols = masks[0].size
    size = -(-cols // BLOCK) * BLOCK
    n = int(sum(int(m.sum()) for m in masks))

    def ordered(term):
        acc = np.zeros(rows[0].shape[:-1] + (size,))
        for x, m in zip(rows, masks):
            acc[..., :cols] = np.where(m, acc[..., :cols] + term(x), acc[..., :cols])
        return _reduce(acc)

    with np.errstate(all="ignore"):
        S = ordered(lambda x: x)
        mean = S / float(n) if n > 0 else S * 0.0
        if mean.ndim:
            M2 = ordered(lambda x: (x - mean[:, None]) * (x - mean[:, None]))
        else:
            M2 = ordered(lambda x: (x - mean) * (x - mean))
    return n, mean, M2


def _merge(na, mean_a, M2_a, nb, mean_b, M2_b):
    """Chan's update in the header's order of roundings; nb > 0."""
    with np.errstate(all="ignore"):
        n = na + nb
        delta = mean_b - mean_a
        w = float(nb) / float(n)
        mean = mean_a + delta * w
        M2 = (M2_a + M2_b) + (delta * delta) * (float(na) * w)
    return n, mean, M2


def fold_obs(rec, obs, done, first, count, learners, skip=None, ended=None):
    L, E, N, F = obs.shape
    assert 0 <= first < count and count - first <= L - 1 and 1 <= F <= MAX_FEATURES and len(rec["mean"]) == F
    rows = [obs[k % L].astype(np.float64).reshape(E * N, F).T for k in range(first, count)]          # [F, columns]
    masks = [sample_mask(done, k, learners, skip, ended).reshape(-1) for k in range(first, count)]
    nb, mean_b, M2_b = _batch(rows, masks)
    if nb == 0:
        return dict(rec)
    n, mean, M2 = _merge(rec["n_obs"], rec["mean"], rec["M2"], nb, mean_b, M2_b)
    return dict(rec, n_obs=n, mean=mean, M2=M2)


def returns(carry, rew, done, first, count, gamma, learners, skip=None, ended=None):
    """The forward walk alone: (R per step oldest first [columns], sample masks [columns], the new carry [E, N])."""
    L, E, N = rew.shape
    assert 0 <= first < count and count - first <= L - 1
    sk, en = _flag_rows(done, skip, ended)
    C = carry.astype(np.float64).copy()
    learner = np.broadcast_to((np.arange(N) < learners)[None, :], (E, N))
    rows, masks = [], []
    with np.errstate(all="ignore"):
        for k in range(first, count):
            s = k % L
            m = sample_mask(done, k, learners, skip, ended)
            R = rew[s].astype(np.float64) + float(gamma) * C
            stop = ((done[s] & 1) != 0) | en[s][:, None]
            C = np.where(learner, np.where(m, np.where(stop, 0.0, R), 0.0), C)
            rows.append(R.reshape(-1))
            masks.append(m.reshape(-1))
    return rows, masks, C


def fold_returns(rec, carry, rew, done, first, count, gamma, learners, skip=None, ended=None):
    rows, masks, C = returns(carry, rew, done, first, count, gamma, learners, skip, ended)
    nb, mean_b, M2_b = _batch(rows, masks)
    if nb == 0:
        return dict(rec), C
    n, mean, M2 = _merge(rec["n_ret"], rec["mean_ret"], rec["M2_ret"], nb, mean_b, M2_b)
    return dict(rec, n_ret=n, mean_ret=float(mean), M2_ret=float(M2)), C


def _clamp(y, clip):
    c = np.float32(clip)
    return np.where(y > c, c, np.where(y < -c, -c, y)).astype(np.float32)


def variances(rec):
    """(mean [F], var [F], var_ret) as the apply calls read the record."""
    with np.errstate(all="ignore"):
        if rec["n_obs"] > 0:
            mean, var = rec["mean"], rec["M2"] / float(rec["n_obs"])
        else:
            mean, var = np.zeros_like(rec["mean"]), np.ones_like(rec["M2"])
        var_ret = rec["M2_ret"] / float(rec["n_ret"]) if rec["n_ret"] > 0 else 1.0
    return mean, var, var_ret


def apply_obs(rec, x, eps=1e-8, clip=10.0):
    """x [..., F] float32 -> float32."""
    mean, var, _ = variances(rec)
    with np.errstate(all="ignore"):
        z = (x.astype(np.float64) - mean) / np.sqrt(var + float(eps))
        return _clamp(z.astype(np.float32), clip)


def scale_rewards(rec, r, eps=1e-8, clip=10.0):
    _, _, var = variances(rec)
    with np.errstate(all="ignore"):
        z = r.astype(np.float64) / np.sqrt(np.float64(var) + float(eps))
        return _clamp(z.astype(np.float32), clip)


# ---- the second writing: one column at a time, Python floats ---------------------------------------------------------------

def _is_sample_loop(done, k, e, i, learners, skip, ended):
    L = done.shape[0]
    packed = skip is None and ended is None

    def is_skip(k):
        return bool(done[k % L, e, 0] & 2) if packed else bool(skip[k % L, e])

    def is_ended(k):
        return bool(done[k % L, e, 0] & 4) if packed else bool(ended[k % L, e])

    if i >= learners or is_skip(k):
        return False
    if k >= 1 and (done[(k - 1) % L, e, i] & 1) and not is_skip(k - 1) and not is_ended(k - 1):
        return False
    return True


def _tree_loop(x):
    """x: 256 floats of one workgroup -> its sum."""
    waves = []
    for w in range(BLOCK // WAVE):
        lane = list(x[w * WAVE:(w + 1) * WAVE])
        off = WAVE // 2
        while off:
            for l in range(off):
                lane[l] = lane[l] + lane[l + off]
            off //= 2
        waves.append(lane[0])
    r = waves[0]
    for w in waves[1:]:
        r = r + w
    return r


def _total_loop(column_sums):
    """column_sums: one float per column, in column order -> the total in the header's order."""
    cols = len(column_sums)
    partial = []
    for blk in range(-(-cols // BLOCK)):
        x = [0.0] * BLOCK
        for t in range(BLOCK):
            if blk * BLOCK + t < cols:
                x[t] = column_sums[blk * BLOCK + t]
        partial.append(_tree_loop(x))
    x = [0.0] * BLOCK
    for j, p in enumerate(partial):
        x[j % BLOCK] = x[j % BLOCK] + p
    return _tree_loop(x)


def _batch_loop(samples):
    """samples: per column, the list of its samples oldest first (Python floats).  (n_b, mean_b, M2_b)."""
    n = sum(len(c) for c in samples)

    def column_sums(term):
        out = []
        for c in samples:
            a = 0.0
            for x in c:
                a = a + term(x)
            out.append(a)
        return out

    S = _total_loop(column_sums(lambda x: x))
    mean = S / n if n > 0 else 0.0
    M2 = _total_loop(column_sums(lambda x: (x - mean) * (x - mean)))
    return n, mean, M2


def _merge_loop(na, mean_a, M2_a, nb, mean_b, M2_b):
    n = na + nb
    delta = mean_b - mean_a
    w = nb / n
    t1 = M2_a + M2_b
    t2 = delta * delta
    t3 = na * w
    return n, mean_a + delta * w, t1 + t2 * t3


def fold_obs_loop(rec, obs, done, first, count, learners, skip=None, ended=None):
    L, E, N, F = obs.shape
    out = dict(rec, mean=rec["mean"].copy(), M2=rec["M2"].copy())
    n_new = rec["n_obs"]
    for f in range(F):
        samples = [[float(obs[k % L, e, i, f]) for k in range(first, count)
                    if _is_sample_loop(done, k, e, i, learners, skip, ended)] for e in range(E) for i in range(N)]
        nb, mean_b, M2_b = _batch_loop(samples)
        if nb == 0:
            continue
        n_new, out["mean"][f], out["M2"][f] = _merge_loop(rec["n_obs"], float(rec["mean"][f]), float(rec["M2"][f]), nb, mean_b,
                                                          M2_b)
    out["n_obs"] = n_new
    return out


def fold_returns_loop(rec, carry, rew, done, first, count, gamma, learners, skip=None, ended=None):
    L, E, N = rew.shape
    packed = skip is None and ended is None
    C_out = carry.astype(np.float64).copy()
    samples = []
    for e in range(E):
        for i in range(N):
            col = []
            if i < learners:
                C = float(carry[e, i])
                for k in range(first, count):
                    if not _is_sample_loop(done, k, e, i, learners, skip, ended):
                        C = 0.0
                        continue
                    R = float(rew[k % L, e, i]) + float(gamma) * C
                    col.append(R)
                    env_ended = bool(done[k % L, e, 0] & 4) if packed else bool(ended[k % L, e])
                    C = 0.0 if (done[k % L, e, i] & 1) or env_ended else R
                C_out[e, i] = C
            samples.append(col)
    nb, mean_b, M2_b = _batch_loop(samples)
    if nb == 0:
        return dict(rec), C_out
    n, mean, M2 = _merge_loop(rec["n_ret"], rec["mean_ret"], rec["M2_ret"], nb, mean_b, M2_b)
    return dict(rec, n_ret=n, mean_ret=mean, M2_ret=M2), C_out


def apply_obs_loop(rec, x, eps=1e-8, clip=10.0):
    F = x.shape[-1]
    flat = x.reshape(-1, F)
    out = np.zeros(flat.shape, np.float32)
    c = np.float32(clip)
    for f in range(F):
        mean = float(rec["mean"][f]) if rec["n_obs"] > 0 else 0.0
        var = float(rec["M2"][f]) / rec["n_obs"] if rec["n_obs"] > 0 else 1.0
        s = var + eps
        den = math.sqrt(s) if s >= 0 else math.nan
        for j in range(flat.shape[0]):
            v = float(flat[j, f])
            with np.errstate(all="ignore"):
                y = np.float32((v - mean) / den) if den != 0 else np.float32(np.float64(v - mean) / np.float64(den))
            out[j, f] = c if y > c else (-c if y < -c else y)
    return out.reshape(x.shape)


def scale_rewards_loop(rec, r, eps=1e-8, clip=10.0):
    var = rec["M2_ret"] / rec["n_ret"] if rec["n_ret"] > 0 else 1.0
    s = var + eps
    den = math.sqrt(s) if s >= 0 else math.nan
    flat = r.reshape(-1)
    out = np.zeros(flat.shape, np.float32)
    c = np.float32(clip)
    for j in range(flat.size):
        v = float(flat[j])
        with np.errstate(all="ignore"):
            y = np.float32(v / den) if den != 0 else np.float32(np.float64(v) / np.float64(den))
        out[j] = c if y > c else (-c if y < -c else y)
    return out.reshape(r.shape)

"""GAE(λ) over the ring and its normalisation, restated from include/uavx_gae.h for the tests.

gae() is the numpy restatement: float64, vectorised over the columns, sequential in k.  stats() sums in the header's
documented order (column sums in walk order, a halving tree over each 64 columns, four wavefronts left to right, then
thread t of one workgroup over partials t, t + 256, ...).  gae_loop() and stats_loop() are a second writing of the same
prose, one column and one Python float at a time, sharing no code with the first.  Rows outside the window keep `fill`."""
import math

import numpy as np

BLOCK, WAVE = 256, 64


def same(a, b):
    """Bit equality, a NaN matching any NaN (the header leaves a NaN's payload and sign open)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))))


def flag_rows(done, skip=None, ended=None):
    """(skip [L,E] bool, ended [L,E] bool) of either flag layout: skip / ended arrays, or bits 1 and 2 of done[:, :, 0]."""
    if (skip is None) != (ended is None):
        raise ValueError("skip and ended come together")
    if skip is None:
        return (done[:, :, 0] & 2) != 0, (done[:, :, 0] & 4) != 0
    return skip != 0, ended != 0


def window_slots(count, steps, L):
    """The window's slots in the order of the walk: k = count − 1 downwards."""
    return [k % L for k in range(count - 1, count - steps - 1, -1)]


def gae(rew, done, values, count, steps, gamma, lam, learners, skip=None, ended=None, fill=0):
    L, E, N = rew.shape
    assert count >= 1 and 1 <= steps <= min(count, L - 1)
    sk, en = flag_rows(done, skip, ended)
    adv = np.full((L, E, N), fill, np.float32)
    ret = np.full((L, E, N), fill, np.float32)
    valid = np.full((L, E, N), fill, np.uint8)
    gl = float(gamma) * float(lam)
    carry = np.zeros((E, N), np.float64)
    learner = (np.arange(N) < learners)[None, :]
    with np.errstate(all="ignore"):
        for k in range(count - 1, count - steps - 1, -1):
            s, s1 = k % L, (k + 1) % L
            d = (done[s] & 1) != 0
            V = values[s].astype(np.float64)
            b = np.where(d, 0.0, float(gamma) * values[s1].astype(np.float64))
            delta = (rew[s].astype(np.float64) + b) - V
            cut = np.ones(E, bool) if k + 1 >= count else sk[s1]
            stop = d | en[s][:, None] | cut[:, None]
            A = np.where(stop, delta, delta + gl * carry)
            live = ~sk[s][:, None] & learner
            adv[s] = np.where(live, A.astype(np.float32), np.float32(0))
            ret[s] = np.where(live, (A + V).astype(np.float32), np.float32(0))
            valid[s] = live
            carry = np.where(sk[s][:, None], 0.0, A)
    return adv, ret, valid


def _workgroup_sum(x):
    """x [blocks, 256] float64 -> [blocks]: the halving tree over each 64 lanes, then w0 + w1 + w2 + w3."""
    w = x.reshape(x.shape[0], BLOCK // WAVE, WAVE)
    off = WAVE // 2
    while off:
        w = w[..., :off] + w[..., off:2 * off]
        off //= 2
    w = w[..., 0]
    r = w[:, 0]
    for j in range(1, BLOCK // WAVE):
        r = r + w[:, j]
    return r


def _total(partial):
    """Thread t adds partial[t], partial[t + 256], ... from +0 in index order; then the workgroup sum."""
    pad = (-len(partial)) % BLOCK
    p = np.concatenate([partial, np.zeros(pad)]).reshape(-1, BLOCK)
    t = np.zeros(BLOCK)
    for row in p:
        t = t + row
    return _workgroup_sum(t[None, :])[0]


def _column_sums(terms, valid, slots):
    """terms, valid [L, E, N]; per column, from +0, the valid terms in the order of `slots`; padded to whole workgroups."""
    cols = terms[0].size
    blocks = -(-cols // BLOCK)
    acc = np.zeros(blocks * BLOCK)
    for s in slots:
        t = terms[s].reshape(-1)
        acc[:cols] = np.where(valid[s].reshape(-1) != 0, acc[:cols] + t, acc[:cols])
    return acc.reshape(blocks, BLOCK)


def stats(adv, valid, count, steps):
    """(n, mean, std) over the window's valid entries of the float32 adv, in the header's order."""
    slots = window_slots(count, steps, adv.shape[0])
    a = adv.astype(np.float64)
    n = int(sum(int((valid[s] != 0).sum()) for s in slots))
    with np.errstate(all="ignore"):
        S = _total(_workgroup_sum(_column_sums(a, valid, slots)))
        mean = S / float(n) if n > 0 else 0.0
        dev = a - mean
        Q = _total(_workgroup_sum(_column_sums(dev * dev, valid, slots)))
        std = math.sqrt(Q / float(n - 1)) if n >= 2 else 0.0     # math.sqrt passes a NaN and +inf through
    return n, float(mean), float(std)


def normalise(adv, valid, count, steps, fill=0):
    """(adv_norm [L,E,N] float32, (n, mean, std)); rows outside the window keep `fill`."""
    n, mean, std = stats(adv, valid, count, steps)
    out = np.full(adv.shape, fill, np.float32)
    with np.errstate(all="ignore"):
        for s in window_slots(count, steps, adv.shape[0]):
            z = ((adv[s].astype(np.float64) - mean) / (std + 1e-8)).astype(np.float32)
            out[s] = np.where(valid[s] != 0, z, np.float32(0))
    return out, (n, mean, std)


# ---- the second writing: one column at a time, Python floats ---------------------------------------------------------------

def _f32(x):
    with np.errstate(all="ignore"):
        return np.float32(x)


def gae_loop(rew, done, values, count, steps, gamma, lam, learners, skip=None, ended=None, fill=0):
    L, E, N = rew.shape
    packed = skip is None and ended is None
    if not packed and (skip is None or ended is None):
        raise ValueError("skip and ended come together")

    def is_skip(k, e):
        return bool(done[k % L, e, 0] & 2) if packed else bool(skip[k % L, e])

    def is_ended(k, e):
        return bool(done[k % L, e, 0] & 4) if packed else bool(ended[k % L, e])

    adv = np.full((L, E, N), fill, np.float32)
    ret = np.full((L, E, N), fill, np.float32)
    valid = np.full((L, E, N), fill, np.uint8)
    gamma_lambda = float(gamma) * float(lam)
    for e in range(E):
        for i in range(N):
            a_plus = 0.0
            for k in range(count - 1, count - steps - 1, -1):
                s, s1 = k % L, (k + 1) % L
                if i >= learners or is_skip(k, e):
                    adv[s, e, i], ret[s, e, i], valid[s, e, i] = 0.0, 0.0, 0
                    a_plus = 0.0
                    continue
                v = float(values[s, e, i])
                if done[s, e, i] & 1:
                    b, stop = 0.0, True
                else:
                    b = float(gamma) * float(values[s1, e, i])
                    stop = is_ended(k, e) or k + 1 >= count or is_skip(k + 1, e)
                delta = (float(rew[s, e, i]) + b) - v
                A = delta if stop else delta + gamma_lambda * a_plus
                adv[s, e, i], ret[s, e, i], valid[s, e, i] = _f32(A), _f32(A + v), 1
                a_plus = A
    return adv, ret, valid


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


def _sum_loop(term, adv, valid, slots):
    """Σ term(a) over the valid entries, in the header's order."""
    E, N = adv.shape[1:]
    cols = E * N
    blocks = -(-cols // BLOCK)
    partial = []
    for blk in range(blocks):
        x = [0.0] * BLOCK
        for t in range(BLOCK):
            q = blk * BLOCK + t
            if q >= cols:
                continue
            e, i = divmod(q, N)
            for s in slots:
                if valid[s, e, i]:
                    x[t] = x[t] + term(float(adv[s, e, i]))
        partial.append(_tree_loop(x))
    x = [0.0] * BLOCK
    for j, p in enumerate(partial):
        x[j % BLOCK] = x[j % BLOCK] + p
    return _tree_loop(x)


def stats_loop(adv, valid, count, steps):
    slots = window_slots(count, steps, adv.shape[0])
    n = sum(1 for s in slots for v in valid[s].reshape(-1) if v)
    S = _sum_loop(lambda a: a, adv, valid, slots)
    mean = S / n if n > 0 else 0.0
    Q = _sum_loop(lambda a: (a - mean) * (a - mean), adv, valid, slots)
    std = math.sqrt(Q / (n - 1)) if n >= 2 else 0.0
    return n, mean, std

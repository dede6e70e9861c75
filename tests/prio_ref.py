"""numpy restatement of prioritized replay (include/uavx_prio.h), written from the header's prose: the refresh of the
priority table, the proportional draw with its gather, and the feedback of TD errors.  The reference the GPU tests of
PrioritizedReplaySampler compare against; test_prio_host.py checks it against per-entry loops on the CPU.

The table is uint32 [L, E, NL] in Q16.16 and every sum is uint64, so the draw is a FLAT cumulative sum and a searchsorted:
no hierarchy appears here, and none can change a bit of the result."""
import collections

import numpy as np

ONE = 65536
P_TOP = 2 ** 32 - 1

Record = collections.namedtuple("Record", "total p_min p_max seen valid")
Sample = collections.namedtuple("Sample", "state action reward next_state mask truncated ended key weight flat")


def new_record():
    return Record(total=0, p_min=0, p_max=ONE, seen=0, valid=0)


def window(count, L):
    """(c, lo) of the header: c = max(1, count), lo = max(0, c − T) with T = L − 1."""
    c = max(int(count), 1)
    return c, max(0, c - (L - 1))


def steps_of_slots(count, L):
    """k [L]: the step slot s belongs to, lo + ((s − lo) mod L); the slot is inside the window where k < c."""
    c, lo = window(count, L)
    return lo + (np.arange(L, dtype=np.int64) - lo) % L


def skip_rows(done, skip):
    """[L, E] bool: the skip flag array, or bit 1 of agent 0's done byte when the flags are packed."""
    return (done[:, :, 0] & 2) != 0 if skip is None else np.asarray(skip) != 0


def refresh(table, rec, count, done, skip=None):
    """-> (table, record) after uavx_prio_refresh.  table [L, E, NL] uint32; done [L, E, N] uint8; skip [L, E] or None."""
    table = np.array(table, dtype=np.uint32)
    L = table.shape[0]
    c, lo = window(count, L)
    k = steps_of_slots(count, L)[:, None, None]
    gone = (k >= c) | skip_rows(done, skip)[:, :, None]
    fresh = ~gone & (k >= max(rec.seen, lo))
    table = np.where(gone, np.uint32(0), np.where(fresh, np.uint32(rec.p_max), table)).astype(np.uint32)
    pos = table[table > 0]
    return table, Record(total=int(table.sum(dtype=np.uint64)), p_min=int(pos.min()) if pos.size else 0, p_max=rec.p_max,
                         seen=c, valid=int(pos.size))


def targets(u, total, stratified):
    """The header's target per row, as Python integers: floor(t · (double)total) clamped into [0, total − 1]."""
    u = np.asarray(u, dtype=np.float32)
    rows = u.shape[0]
    out = []
    for j in range(rows):
        uj = float(u[j])
        with np.errstate(all="ignore"):
            t = (float(j) + uj) / float(rows) if stratified else uj
        if not t > 0.0:                      # NaN and negatives
            out.append(0)
        elif t >= 1.0:                       # +inf too
            out.append(total - 1)
        else:
            out.append(min(total - 1, int(np.floor(np.float64(t) * np.float64(total)))))
    return out


def sample(u, table, rec, count, obs, act, rew, done, skip=None, trunc=None, ended=None, stratified=True, beta=0.4):
    """uavx_prio_sample on a refreshed table and its record.  u [rows] float32; beta a float32 value."""
    table = np.asarray(table, dtype=np.uint32)
    L, E, NL = table.shape
    rows = len(u)
    c, lo = window(count, L)
    per_slot = E * NL
    if skip is None:
        trunc, ended = (done[:, :, 0] & 8) != 0, (done[:, :, 0] & 4) != 0
    else:
        trunc, ended = np.asarray(trunc) != 0, np.asarray(ended) != 0
    if rec.total == 0:
        s = np.full(rows, (c - 1) % L, dtype=np.int64)
        e = i = np.zeros(rows, dtype=np.int64)
        flat = np.full(rows, -1, dtype=np.int64)
        key = np.full(rows, -1, dtype=np.int64)
        weight = np.zeros(rows, dtype=np.float32)
    else:
        cum = np.cumsum(table.reshape(-1), dtype=np.uint64)
        assert int(cum[-1]) == rec.total
        flat = np.searchsorted(cum, np.array(targets(u, rec.total, stratified), dtype=np.uint64), side="right").astype(np.int64)
        s, rest = flat // per_slot, flat % per_slot
        e, i = rest // NL, rest % NL
        key = steps_of_slots(count, L)[s] * per_slot + rest
        p = table.reshape(-1)[flat].astype(np.float64)
        weight = np.power(np.float64(rec.p_min) / p, np.float64(np.float32(beta))).astype(np.float32)
    s1 = (s + 1) % L
    mask = np.float32(1.0) - (done[s, e, i] & 1).astype(np.float32)
    return Sample(obs[s, e, i], act[s, e, i], rew[s, e, i], obs[s1, e, i], mask, trunc[s, e], ended[s, e], key, weight, flat)


def priority(delta, alpha, eps):
    """p of the header for float32 |TD errors|: NaN gives 1 and +inf the top for every alpha; otherwise
    floor(pow((double)delta + eps, alpha)·65536 + 0.5) clamped into [1, 2^32 − 1]."""
    d = np.asarray(delta, dtype=np.float32).astype(np.float64) + np.float64(eps)
    with np.errstate(all="ignore"):
        x = (d if alpha == 1.0 else np.ones_like(d) if alpha == 0.0 else np.power(d, np.float64(alpha))) * 65536.0 + 0.5
    x = np.where(np.isnan(d), np.nan, np.where(np.isposinf(d), np.inf, x))       # settled first, whatever alpha
    p = np.ones(x.shape, dtype=np.uint64)
    big = x >= 4294967295.0
    mid = (x >= 1.0) & ~big
    p[big] = P_TOP
    p[mid] = np.floor(x[mid]).astype(np.uint64)
    return p.astype(np.uint32)


def delta_of(q, y=None):
    """max over the towers of |q_t − y| in float32, a NaN in any tower staying; q [towers, rows], y [rows] or None."""
    q = np.asarray(q, dtype=np.float32).reshape(-1, np.asarray(q).shape[-1])
    with np.errstate(all="ignore"):
        d = np.abs(q) if y is None else np.abs(q - np.asarray(y, dtype=np.float32).reshape(1, -1))
        out = d.max(axis=0)                  # numpy's max hands a NaN on
    return out.astype(np.float32)


def update(table, rec, count, key, q, y=None, alpha=0.6, eps=1e-6):
    """-> (table, record) after uavx_prio_update: the sums of the record are NOT rebuilt, only p_max moves."""
    table = np.array(table, dtype=np.uint32)
    L, E, NL = table.shape
    c, lo = window(count, L)
    per_slot = E * NL
    key = np.asarray(key, dtype=np.int64)
    p = priority(delta_of(q, y), alpha, eps)
    k = key // per_slot
    live = (key >= 0) & (k >= lo) & (k < c)
    flat = (k[live] % L) * per_slot + key[live] % per_slot
    t = table.reshape(-1)
    t[flat] = 0
    np.maximum.at(t, flat, p[live])
    p_max = max(rec.p_max, int(p[live].max())) if live.any() else rec.p_max
    return table, rec._replace(p_max=p_max)

"""Crafted neighbour layouts for the 6-64 UAV neighbour key scan (scan_neighbours of csrc/uavx_multi_scan.hpp, N > 5 and the
8-UAV specialisation), and a host model of its integer key arithmetic (numpy only).

The device arithmetic (float32, no FMA: neighbour_layouts.squares) is restated as it is written in the kernel:
  key  = (bits(s) & ~63) | c       s the squared distance to the neighbour, c its rank among the OTHER slots of the env as seen
                                   from agent i (slot j = c + (c >= i))
  k1 <= k2 <= k3                   the three smallest keys, t = k >> 6 their truncation buckets, ts = bits(sq_sense) >> 6
  near_tie = (t2 - t1 <= 1 and t1 <= ts) or (t3 - t2 <= 1 and t2 <= ts)
A lane that is no near tie reports the slots named by k1 and k2, each if its own square is < sq_sense (key_path()).  A near tie
is resolved exactly: by the whole wavefront for that lane while at most 6 lanes of the wavefront tie, by the compare / select
scan of every lane from 7 on.  A workgroup of W wavefronts (group_waves(): the table of pick_group_waves()) holds
epw = floor(64 W / N) whole envs, thread = (e % epw) N + i, wavefront thread // 64 of the workgroup; the two tiles of an 8-UAV
workgroup are wavefronts 2 g and 2 g + 1, i.e. the wavefronts of the one-tile launch.  tied_lanes_per_wave() counts the near
ties of every wavefront.  The TRUTH is not this model but neighbour_layouts.nearest_two: order by (float32 root, slot).

make_batch() crafts one ego per cluster (ego + the 0-4 neighbours the class needs, every other slot of the env in range but
>= 4 buckets away from the crafted squares, or well out of range); classify() recomputes the classes from the positions:
  A2 A3 A4   exact square ties among the nearest two / three / four (A4: an agent outside the kept three at the tie)
  B  B'      1st and 2nd (B': 2nd and 3rd) in ONE bucket, different roots, the lower rank on the larger square
  C  C'      1st and 2nd (C': 2nd and 3rd) in ADJACENT buckets, 1-4 ulps apart, equal roots, the lower slot on the larger square
  D12 D23    buckets exactly 2 apart, 65-128 ulps, the lower rank on the larger square: the fast path just past the threshold
  F-1 F0 F+1 a single neighbour at sq_sense - 1 ulp, sq_sense, sq_sense + 1 ulp
  Ftie-a Ftie-a'  B / B' inside the bucket ts, both squares < sq_sense (needs two squares with different roots there)
  Ftie-b     one square < sq_sense <= the other, same bucket (the lower rank out of range) or adjacent buckets
  Ftie-c     the nearest two at or just above sq_sense in the bucket ts: a near tie whose answer is "no neighbour"
  G0 G1      nobody / exactly one in range, the other kept keys far out of range
  I          ego index 0, 1, n-2 or n-1 with the winners at slots i-1 and i+1 or at slots 0 and n-1 (rank -> slot mapping)
Wavefront plan (make_batch()["plan"]: wavefront -> kind), repeated with the classes rotating through it:
  zero   no tied lane          first  lane 0 alone           last   the last active lane alone
  pair   two tied lanes of one env                            six / seven   exactly 6 / 7 tied lanes
  all    every lane tied (regular polygons, as reset(circular=True) draws them); a whole workgroup at a time
and a ragged last workgroup.  Every agent gets a distinct heading, so a wrong neighbour moves observation column 6 / 9 by at
least 1.2 / slots."""
import math

import numpy as np

from neighbour_layouts import F32, _grid, bits, sq_limit_lt, squares

WAVE = 64
AGENTS = (6, 7, 8, 10, 13, 24, 64)
SENSE = (9.0, 15.0, 7.3, 6.1)   # bits(sq_limit_lt(d)) & 63 = 63, 0, 54, 10: the limit at the top / bottom of / inside its bucket
WORLD = dict(x_size=600.0, y_size=600.0)
EXT_SLOTS = 192                 # kExtSlots: neighbour rows of one wavefront of the kernels with scripted bodies

# pick_group_waves() of csrc/uavx_multi_launch.hpp: its table, copied as data (agent counts outside it are not used here)
GROUP_WAVES = {1: 1, 2: 1, 4: 1, 5: 1, 8: 1, 3: 3, 6: 3, 7: 3, 11: 3, 12: 3, 24: 3, 48: 3, 9: 2, 10: 2, 15: 2, 20: 2, 40: 2,
               13: 1, 14: 1, 16: 1, 28: 1, 32: 1, 64: 1}

TIED = ("A2", "A3", "A4", "B", "B'", "C", "C'", "Ftie-a", "Ftie-a'", "Ftie-b", "Ftie-c")
UNTIED = ("D12", "D23", "F-1", "F0", "F+1", "G0", "G1", "I")
SATS = {"A2": 2, "A3": 3, "A4": 4, "B": 2, "B'": 3, "C": 2, "C'": 3, "D12": 2, "D23": 3, "F-1": 1, "F0": 1, "F+1": 1,
        "Ftie-a": 2, "Ftie-a'": 3, "Ftie-b": 2, "Ftie-c": 2, "G0": 0, "G1": 1, "I": 2}
KINDS = ("zero", "first", "last", "pair", "six", "seven")


def group_waves(n):
    return GROUP_WAVES[n]


def envs_per_group(n, W, bodies=0):
    return min(WAVE * W // n, EXT_SLOTS // (n + bodies))


# ---------------------------------------------------------------------------------------------------------------------------
# host model
def all_squares(loc):
    """[E, S, S] float32: S[e, i, j] = squared distance from slot i to slot j as the device computes it (a slot at +inf: +inf)."""
    loc = np.asarray(loc, F32)
    with np.errstate(invalid="ignore"):
        d = loc[:, None, :, :] - loc[:, :, None, :]
        s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    return np.where(np.isnan(s), F32(np.inf), s).astype(F32)


def _others(n):
    return np.array([[j for j in range(n) if j != i] for i in range(n)])   # [n, n - 1]: slot of rank c as seen from i


def keys_of(S):
    """[E, S, S - 1] uint32 keys of every lane, rank c along the last axis."""
    n = S.shape[1]
    so = S[:, np.arange(n)[:, None], _others(n)]
    return (so.view(np.uint32) & np.uint32(0xFFFFFFC0)) | np.arange(n - 1, dtype=np.uint32)


def three_smallest(keys):
    return np.sort(keys, axis=-1)[..., :3].astype(np.int64)


def _per_env(x, E):
    return np.broadcast_to(np.asarray(x, F32).reshape(-1, 1), (E, 1))


def near_tie(loc, sq_sense):
    """[E, S] bool: the kernel's predicate, exactly as written.  sq_sense: scalar or [E] (levels)."""
    S = all_squares(loc)
    k = three_smallest(keys_of(S))
    t1, t2, t3 = k[..., 0] >> 6, k[..., 1] >> 6, k[..., 2] >> 6
    ts = bits(_per_env(sq_sense, S.shape[0])) >> 6
    tie = ((t2 - t1 <= 1) & (t1 <= ts)) | ((t3 - t2 <= 1) & (t2 <= ts))
    return tie & np.isfinite(np.asarray(loc, F32)).all(-1)          # a parked slot (+inf) has NaN keys: never tied


def key_path(loc, sq_sense):
    """[E, S, 2] slots the key order ALONE reports (-1: none): what the kernel returns for a lane that is no near tie."""
    S = all_squares(loc)
    E, n = S.shape[:2]
    k = three_smallest(keys_of(S))
    out = np.full((E, n, 2), -1, np.int64)
    sq = _per_env(sq_sense, E)
    i = np.arange(n)[None]
    for r in range(2):
        c = k[..., r] & 63
        j = c + (c >= i)
        s = np.take_along_axis(S, j[..., None], -1)[..., 0]
        out[..., r] = np.where(s < sq, j, -1)
    return out


def truth(loc, sq_sense):
    """([E, S, 2] slots, [E, S, 2] float32 roots) ordered by (float32 root, slot) among the squares < sq_sense: nearest_two of
    neighbour_layouts for every lane at once (-1 / inf: none)."""
    S = all_squares(loc)
    E, n = S.shape[:2]
    oth = _others(n)
    so = S[:, np.arange(n)[:, None], oth]
    root = np.where(so < _per_env(sq_sense, E)[..., None], np.sqrt(so), F32(np.inf))
    order = np.argsort(root, axis=-1, kind="stable")[..., :2]
    d = np.take_along_axis(root, order, -1)
    j = np.broadcast_to(oth[None], so.shape)
    j = np.take_along_axis(j, order, -1)
    return np.where(np.isfinite(d), j, -1), d


def lane_table(E, n, W, epw=None):
    """([E, n] wavefront of the launch, [E, n] lane) of every agent: n lanes per env (learners), epw envs per workgroup."""
    epw = epw or envs_per_group(n, W)
    e, i = np.arange(E)[:, None], np.arange(n)[None]
    thread = (e % epw) * n + i
    return (e // epw) * W + thread // WAVE, thread % WAVE


def tied_lanes_per_wave(loc, n, d_sense, W, epw=None):
    """[wavefronts] number of near-tie lanes.  loc [E, S, 2] with S >= n slots (slots from n on are bodies without a lane);
    d_sense scalar or [E]."""
    loc = np.asarray(loc, F32)
    E = loc.shape[0]
    sq = np.array([sq_limit_lt(d) for d in np.broadcast_to(np.asarray(d_sense, np.float64), (E,))], F32)
    tie = near_tie(loc, sq)[:, :n]
    wave, _ = lane_table(E, n, W, epw or envs_per_group(n, W, loc.shape[1] - n))
    return np.bincount(wave.ravel(), weights=tie.ravel(), minlength=int(wave.max()) + 1).astype(np.int64)


def active_lanes_per_wave(E, n, W, epw=None):
    wave, _ = lane_table(E, n, W, epw)
    return np.bincount(wave.ravel(), minlength=int(wave.max()) + 1)


# ---------------------------------------------------------------------------------------------------------------------------
# classes
def _roots_differ_in_limit_bucket(sq):
    """Two squares < sq_sense of the bucket ts with different float32 roots exist."""
    bs = int(bits(sq))
    b = np.arange(bs & ~63, bs, dtype=np.uint32)
    return b.size >= 2 and np.unique(np.sqrt(b.view(F32))).size >= 2


def classes_possible(n, d_sense):
    """(possible, impossible): every class is in exactly one of the two lists, the impossible ones with the reason."""
    sq = sq_limit_lt(d_sense)
    poss, imposs = list(TIED + UNTIED), {}
    if not _roots_differ_in_limit_bucket(sq):
        for c in ("Ftie-a", "Ftie-a'"):
            poss.remove(c)
            imposs[c] = f"bits(sq_sense) & 63 = {int(bits(sq)) & 63}: no two squares below the limit in its bucket"
    return poss, imposs


def classify(loc_env, i, sq_sense, slots=None):
    """The set of class tags of agent i, from the positions alone.  slots: the env's slots that take part (default: all)."""
    n = loc_env.shape[0]
    s_all = squares(loc_env[i], loc_env)
    nb = sorted((F32(s_all[j]), j) for j in (range(n) if slots is None else slots) if j != i and np.isfinite(s_all[j]))
    sb = [int(bits(s)) for s, _ in nb]
    tb = [b >> 6 for b in sb]
    rt = [F32(np.sqrt(s)) for s, _ in nb]
    js = [j for _, j in nb]
    bs = int(bits(sq_sense))
    ts = bs >> 6
    m = len(nb)
    tags = set()
    gap = lambda a: a + 1 >= m or tb[a + 1] - tb[a] >= 4          # the neighbour behind position a is >= 4 buckets away
    inr = [b < bs for b in sb]
    if m >= 2 and sb[0] == sb[1] and inr[1]:
        tags.add("A2")
    if m >= 3 and sb[0] == sb[1] == sb[2] and inr[2]:
        tags.add("A3")
    if m >= 4 and sb[0] == sb[1] == sb[2] == sb[3] and inr[3]:
        tags.add("A4")
    for a, tag in ((0, ""), (1, "'")):
        if m < a + 2 or not inr[a + 1] or (a == 1 and not tb[1] - tb[0] >= 4):
            continue
        lo, hi = a, a + 1
        inverted = js[hi] < js[lo]
        if tb[lo] == tb[hi] and sb[lo] < sb[hi] and rt[lo] != rt[hi] and inverted:
            tags.add("B" + tag)
            if tb[lo] == ts:
                tags.add("Ftie-a" + tag)
        if tb[hi] == tb[lo] + 1 and 1 <= sb[hi] - sb[lo] <= 4 and rt[lo] == rt[hi] and inverted:
            tags.add("C" + tag)
        if tb[hi] == tb[lo] + 2 and 65 <= sb[hi] - sb[lo] <= 128 and inverted and gap(hi):
            tags.add("D12" if a == 0 else "D23")
    edge = [b - bs for b in sb if abs(b - bs) <= 256]
    if len(edge) == 1 and abs(edge[0]) <= 1:
        tags.add({-1: "F-1", 0: "F0", 1: "F+1"}[edge[0]])
    if m >= 2 and inr[0] and not inr[1] and tb[1] - tb[0] <= 1:
        tags.add("Ftie-b")
    if m >= 2 and not inr[0] and tb[0] == tb[1] == ts:
        tags.add("Ftie-c")
    nin = sum(inr)
    if nin == 0 and (m == 0 or tb[0] - ts >= 4):
        tags.add("G0")
    if nin == 1 and (m == 1 or tb[1] - ts >= 4) and ts - tb[0] >= 4:
        tags.add("G1")
    if i in (0, 1, n - 2, n - 1) and nin >= 2 and tb[1] - tb[0] >= 4 and gap(1):
        if {js[0], js[1]} <= {i - 1, i + 1, 0, n - 1}:
            tags.add("I")
    return tags


# ---------------------------------------------------------------------------------------------------------------------------
# generator
def _f32_of_bits(b):
    return np.array([b], np.uint32).view(F32)[0]


def _polar(p, ang, r):
    return (p.astype(np.float64) + r * np.array([math.cos(ang), math.sin(ang)])).astype(F32)


def _cluster(rng, cls, p, d_sense, sq):
    """Satellites of an ego at p in class cls: (points, inverted) -- points in ascending order of their squares; inverted: a
    pair (a, b) of positions in that list with slot(b) < slot(a) required -- or None if this draw did not reach the class."""
    K = 40 if float(np.abs(p).max()) < 16 else 160          # coarser float32 grid away from the origin: search more of it
    k = SATS[cls]
    a0 = rng.uniform(-math.pi, math.pi)
    ang = [a0 + (2 * math.pi / max(k, 1)) * (m + rng.uniform(-0.2, 0.2)) for m in range(k)]
    r = float(rng.uniform(0.35, 0.6)) * d_sense
    bs = int(bits(sq))
    lo_b = bs & ~63
    s_of = lambda q: F32(squares(p, q))

    def at(m, pred, around):                                # a point at angle m whose square satisfies pred, searched around a square
        return _grid(p, ang[m], math.sqrt(float(around)), pred, rng, K=K)

    pts, inv = [], None
    first = 0
    if cls in ("B'", "C'", "D23", "Ftie-a'"):               # a clearly nearer first neighbour
        pts.append(_polar(p, ang[0], r * rng.uniform(0.45, 0.6)))
        first = 1
    if cls in ("A2", "A3", "A4"):
        q1 = _polar(p, ang[0], r)
        b1 = int(bits(s_of(q1)))
        pts.append(q1)
        for m in range(1, k):
            pts.append(at(m, lambda s: bits(s) == b1, s_of(q1)))
    elif cls in ("B", "B'"):
        q1 = at(first, lambda s: (bits(s) & 63) <= 40, F32(r * r))
        if q1 is None:
            return None
        s1 = s_of(q1)
        b1 = int(bits(s1))
        q2 = at(first + 1, lambda s: (bits(s) >> 6 == b1 >> 6) & (bits(s) > b1) & (np.sqrt(s) != np.sqrt(s1)), s1)
        pts += [q1, q2]
        inv = (first, first + 1)
    elif cls in ("C", "C'"):
        def shares_root_across_edge(s):                     # a square 1-4 ulps up, in the next bucket, has the same root
            b = bits(s)
            ok = np.zeros(b.shape, bool)
            for m in range(1, 5):
                up = (b + m).astype(np.uint32).view(F32)
                ok |= ((b + m) >> 6 == (b >> 6) + 1) & (np.sqrt(up) == np.sqrt(s))
            return ok
        q1 = at(first, shares_root_across_edge, F32(r * r))
        if q1 is None:
            return None
        s1 = s_of(q1)
        b1 = int(bits(s1))
        q2 = at(first + 1, lambda s: (bits(s) >> 6 == (b1 >> 6) + 1) & (bits(s) - b1 <= 4) & (np.sqrt(s) == np.sqrt(s1)), s1)
        pts += [q1, q2]
        inv = (first, first + 1)
    elif cls in ("D12", "D23"):
        q1 = _polar(p, ang[first], r)
        b1 = int(bits(s_of(q1)))
        q2 = at(first + 1, lambda s: (bits(s) >> 6 == (b1 >> 6) + 2) & (bits(s) - b1 >= 65) & (bits(s) - b1 <= 128),
                _f32_of_bits(b1 + 96))
        pts += [q1, q2]
        inv = (first, first + 1)
    elif cls in ("F-1", "F0", "F+1"):
        tb = bs + {"F-1": -1, "F0": 0, "F+1": 1}[cls]
        pts.append(at(0, lambda s: bits(s) == tb, sq))
    elif cls in ("Ftie-a", "Ftie-a'"):
        q1 = at(first, lambda s: (bits(s) >= lo_b) & (bits(s) <= bs - 2), sq)
        if q1 is None:
            return None
        s1 = s_of(q1)
        b1 = int(bits(s1))
        q2 = at(first + 1, lambda s: (bits(s) > b1) & (bits(s) < bs) & (np.sqrt(s) != np.sqrt(s1)), sq)
        pts += [q1, q2]
        inv = (first, first + 1)
    elif cls == "Ftie-b":
        same = (bs & 63) >= 1 and rng.random() < 0.6
        if same:        # both in the bucket ts
            q1 = at(0, lambda s: (bits(s) >= lo_b) & (bits(s) < bs), sq)
            q2 = at(1, lambda s: (bits(s) >= bs) & (bits(s) <= lo_b + 63), sq)
        elif (bs & 63) == 0:   # the limit opens its bucket: below it is the bucket ts - 1
            q1 = at(0, lambda s: (bits(s) >= bs - 4) & (bits(s) < bs), sq)
            q2 = at(1, lambda s: (bits(s) >= bs) & (bits(s) <= bs + 4), sq)
        else:           # below the limit in ts, the other in the first squares of ts + 1
            q1 = at(0, lambda s: (bits(s) >= max(lo_b, bs - 8)) & (bits(s) < bs), sq)
            q2 = at(1, lambda s: (bits(s) >= lo_b + 64) & (bits(s) <= lo_b + 71), _f32_of_bits(lo_b + 66))
        pts += [q1, q2]
        inv = (0, 1)
    elif cls == "Ftie-c":
        hi = min(bs + 3, lo_b + 63)
        pts.append(at(0, lambda s: bits(s) == bs, sq))
        pts.append(at(1, lambda s: (bits(s) >= bs) & (bits(s) <= hi), sq))
        if pts[0] is not None and pts[1] is not None and bits(s_of(pts[1])) < bits(s_of(pts[0])):
            pts.reverse()
    elif cls == "G1":
        pts.append(_polar(p, ang[0], d_sense * rng.uniform(0.3, 0.9)))
    elif cls == "I":
        pts += [_polar(p, ang[0], r), _polar(p, ang[1], r * rng.uniform(1.15, 1.4))]
    elif cls != "G0":
        raise ValueError(cls)
    if any(q is None for q in pts):
        return None
    return pts, inv


# classes whose ego may have further neighbours in range behind the crafted ones / in front of them
_BEHIND = ("A2", "A3", "A4", "B", "B'", "C", "C'", "D12", "D23", "I")
_FRONT = ("F-1", "F0", "F+1")


def _craft_env(rng, slots, egos, d_sense, sq, n_rows, prefer=None, lanes=None):
    """One env: egos = [(slot, cls, forced satellite slots or None)].  slots: the slots that take part (the others stay at
    +inf).  prefer(slot) -> slots to take the satellites from first.  Returns loc [n_rows, 2] or None."""
    loc = np.full((n_rows, 2), np.inf, F32)
    free = [j for j in slots if j not in [e[0] for e in egos] and not any(e[2] and j in e[2] for e in egos)]
    rng.shuffle(free)
    pitch = 4.5 * d_sense
    cells = [(gx, gy) for gx in range(-1, 2) for gy in range(-1, 2)]
    rng.shuffle(cells)
    centres = []
    for c, (i, cls, forced) in enumerate(egos):
        if len(egos) == 1:
            p = rng.uniform(-8, 8, 2).astype(F32)
        else:
            p = (np.array(cells[c]) * pitch + rng.uniform(-2, 2, 2)).astype(F32)
        got = _cluster(rng, cls, p, d_sense, sq)
        if got is None:
            return None
        pts, inv = got
        if forced:
            take = list(forced)
        else:
            want = [j for j in (prefer(i) if prefer else []) if j in free]
            rng.shuffle(want)
            pool = want + [j for j in free if j not in want]
            if len(pool) < len(pts):
                return None
            take = pool[:len(pts)]
            rng.shuffle(take)
        if inv is not None and not take[inv[1]] < take[inv[0]]:
            take[inv[0]], take[inv[1]] = take[inv[1]], take[inv[0]]
        free = [j for j in free if j not in take]
        loc[i] = p
        for j, q in zip(take, pts):
            loc[j] = q
        centres.append((p, cls, max([float(np.sqrt(squares(p, q))) for q in pts] or [0.0])))
    # in-range fillers, >= 4 buckets (in fact >= 8 %) away from every crafted square
    for p, cls, rmax in centres:
        if cls in _BEHIND and rmax * 1.1 < 0.95 * d_sense:
            for _ in range(int(rng.integers(0, 3))):
                if free:
                    loc[free.pop()] = _polar(p, rng.uniform(-math.pi, math.pi), rng.uniform(rmax * 1.1, 0.95 * d_sense))
        elif cls in _FRONT and rng.random() < 0.5 and free:
            loc[free.pop()] = _polar(p, rng.uniform(-math.pi, math.pi), d_sense * rng.uniform(0.3, 0.8))
    # everybody else well out of range of every ego
    box = 2.0 * pitch
    for j in free:
        for _ in range(1000):
            q = rng.uniform(-box, box, 2).astype(F32)
            if all(float(np.sqrt(squares(p, q))) > 1.4 * d_sense for p, _, _ in centres):
                break
        loc[j] = q
    return loc


def _polygon_env(rng, n, d_sense):
    """A regular n-gon whose sides are well inside the sensing range (every lane ties its two neighbours)."""
    side = d_sense * rng.uniform(0.25, 0.5)
    R = side / (2 * math.sin(math.pi / n))
    a0 = rng.uniform(-math.pi, math.pi)
    c = rng.uniform(-4, 4, 2)
    a = a0 + 2 * math.pi * np.arange(n) / n
    return (c[None] + R * np.stack([np.cos(a), np.sin(a)], -1)).astype(F32)


def _headings(rng, E, slots):
    """[E, slots] distinct headings: slot k points at a0 + 2 pi k / slots (+- 0.2 of that pitch), wrapped into (-pi, pi]."""
    pitch = 2 * math.pi / slots
    a = rng.uniform(-math.pi, math.pi, (E, 1)) + pitch * (np.arange(slots)[None] + rng.uniform(-0.2, 0.2, (E, slots)))
    return np.arctan2(np.sin(a), np.cos(a))


def _budget(n_free, classes):
    return sum(SATS[c] for c in classes) <= n_free


def make_batch(n, d_sense, seed=0, W=None, bodies=0, reps=6, n_active=None, b_active=None, d_env=None, tied=None):
    """Deterministic crafted batch for n lanes per env (learners) and `bodies` further slots without a lane.
    Returns dict(loc [E, n + bodies, 2] f32, vel [E, n, 2] f64, heading [E, n + bodies] (of every slot; bodies take theirs from
    it), ego_env / ego_i / ego_cls / ego_wave / ego_lane (one entry per crafted ego), plan {wavefront: kind}, W, epw, sq_sense,
    d_sense).  n_active / b_active: only these many learners / bodies take part (the others stay at +inf: a level).
    d_env [E]: per-env sensing range (levels) -- E is then fixed by it.  tied: the tied classes to rotate through."""
    W = W or (1 if bodies else group_waves(n))
    S = n + bodies
    rng = np.random.default_rng([seed, n, int(round(d_sense * 1000)), bodies, W])
    epw = envs_per_group(n, W, bodies)
    if d_env is None:
        groups = (len(KINDS) * reps + W - 1) // W + 2          # + one workgroup of polygons + a ragged one
        if n == 8 and groups % 2:
            groups += 1                                        # pairs of tiles need an even number of wavefronts
        E = groups * epw - max(1, epw // 3)
        d_env = np.full(E, float(d_sense))
    else:
        d_env = np.asarray(d_env, np.float64)
        E = len(d_env)
        groups = (E + epw - 1) // epw
    sq_env = np.array([sq_limit_lt(d) for d in d_env], F32)
    wave, lane = lane_table(E, n, W, epw)
    nl = n_active or n
    slots = list(range(nl)) + list(range(n, n + (bodies if b_active is None else b_active)))
    n_waves = int(wave.max()) + 1
    poly_group = groups - 2 if groups >= 3 else -1
    plan, env_egos = {}, {e: [] for e in range(E)}
    poss = [c for c in (tied or TIED) if c in classes_possible(n, d_sense)[0] or d_env.min() != d_env.max()]
    small = [c for c in poss if SATS[c] == 2]

    given = {c: 0 for c in poss}

    def next_tied(e, k_more):
        """The tied class handed out least so far that still fits into env e with k_more further egos to come (2 satellites each)."""
        used = 1 + sum(1 + SATS[c] for _, c, _ in env_egos[e])
        room = len(slots) - used - 3 * k_more
        fits = [c for c in poss if SATS[c] <= room and (d_env.min() == d_env.max() or c in classes_possible(n, d_env[e])[0])]
        if not fits:
            return None
        c = min(fits, key=lambda c: (given[c], -SATS[c], poss.index(c)))
        given[c] += 1
        return c

    kinds_of = {}
    k_idx = 0
    for w in range(n_waves):
        g = w // W
        if g == poly_group:
            kinds_of[w] = "all"
        elif g == groups - 1:
            kinds_of[w] = "zero" if w % 2 else "six"           # the ragged workgroup
        else:
            kinds_of[w] = KINDS[(k_idx + k_idx // len(KINDS)) % len(KINDS)]   # rotate against the wavefront-in-workgroup index
            k_idx += 1
    for w in range(n_waves):
        kind = kinds_of[w]
        here = [(int(e), int(i)) for e, i in zip(*np.nonzero(wave == w)) if i < nl]
        here.sort(key=lambda ei: lane[ei])
        if not here or kind in ("zero", "all"):
            plan[w] = kind if here else "idle"
            continue
        if kind == "first":
            picks = [here[0]]
        elif kind == "last":
            picks = [here[-1]]
        elif kind == "pair":
            inside = [e for e in sorted({e for e, _ in here}) if sum(1 for x in here if x[0] == e) >= min(nl, 2)
                      and len(slots) >= 6]
            e = inside[len(inside) // 2]
            mine = [x for x in here if x[0] == e]
            picks = [mine[0], mine[-1]]
        else:
            want = 6 if kind == "six" else 7
            envs = sorted({e for e, _ in here})
            per_env_max = max(1, len(slots) // 3)
            picks, round_ = [], 0
            while len(picks) < want and round_ < per_env_max:
                for e in envs:
                    mine = [x for x in here if x[0] == e and x not in picks]
                    taken = sum(1 for x in picks if x[0] == e) + len(env_egos[e])
                    if mine and taken < per_env_max and len(picks) < want:
                        picks.append(mine[int(rng.integers(len(mine)))])
                round_ += 1
            if len(picks) < want:                              # a ragged wavefront too small for it
                kind = f"tied{len(picks)}"
        plan[w] = kind
        for idx, (e, i) in enumerate(picks):
            more = sum(1 for x in picks[idx + 1:] if x[0] == e)
            lead = ("B", "C", "Ftie-a")                        # these three in every six / seven wavefront
            c = lead[idx] if kind in ("six", "seven") and idx < 3 and lead[idx] in poss and (
                d_env.min() == d_env.max() or lead[idx] in classes_possible(n, d_env[e])[0]) else next_tied(e, more)
            if c is None:
                raise RuntimeError(f"no tied class fits env {e} at n={n}")
            env_egos[e].append((i, c, None))
    # untied egos: every env without an ego gets one (class I first where envs are few; it sweeps the ego index and takes its
    # winners from slots i - 1, i + 1, 0 and n - 1), and envs with room take up to three more; they change no tied count
    i_sweep, u = 0, 0
    untied = [c for c in UNTIED if c in classes_possible(n, d_sense)[0]]
    plain = [c for c in untied if c != "I"]
    i_slots = {0: ((1, nl - 1),), 1: ((0, 2), (0, nl - 1)), nl - 2: ((nl - 3, nl - 1), (0, nl - 1)), nl - 1: ((0, nl - 2),)}
    for e in range(E):
        if e // epw == poly_group:
            continue
        if not env_egos[e] and nl == S and (n >= 24 or u % len(untied) == len(untied) - 1):
            i = (0, 1, nl - 2, nl - 1)[i_sweep % 4]
            opts = i_slots[i]
            env_egos[e].append((i, "I", opts[(i_sweep // 4) % len(opts)]))
            i_sweep += 1
            u += n < 24
        for extra in range(4):
            used = sum(1 + SATS[c] for _, c, _ in env_egos[e])
            taken = {i for i, _, _ in env_egos[e]} | {j for _, _, f in env_egos[e] if f for j in f}
            lanes_free = [i for i in range(nl) if i not in taken]
            c = plain[u % len(plain)] if plain[u % len(plain)] != "I" else "D12"
            if (env_egos[e] and (extra >= 3 or n < 13)) or len(env_egos[e]) >= 9 or 1 + SATS[c] + 1 > len(slots) - used or not lanes_free:
                break
            env_egos[e].append((lanes_free[int(rng.integers(len(lanes_free)))], c, None))
            u += 1
    # build
    loc = np.full((E, S, 2), np.inf, F32)
    ego_env, ego_i, ego_cls = [], [], []
    for e in range(E):
        if e // epw == poly_group:
            loc[e, slots] = _polygon_env(rng, len(slots), float(d_env[e]))
            continue
        egos = env_egos[e]
        straddle = wave[e].min() != wave[e].max()

        def prefer(i, e=e, straddle=straddle):
            if straddle:                                       # winners in the OTHER wavefront of the env
                return [j for j in slots if j < n and wave[e, j] != wave[e, i]]
            if bodies and (e + i) % 2:
                return [j for j in slots if j >= n]            # ties among / with bodies
            return []
        for attempt in range(400):
            got = _craft_env(rng, slots, egos, float(d_env[e]), sq_env[e], S, prefer)
            if got is None:
                continue
            want = np.zeros(S, bool)
            for i, c, _ in egos:
                want[i] = c in TIED
            if not np.array_equal(near_tie(got[None], sq_env[e])[0][:n], want[:n]):
                continue
            if all(c in classify(got, i, sq_env[e], slots) for i, c, _ in egos):
                break
        else:
            raise RuntimeError(f"could not craft env {e} {egos} at n={n}, d_sense={d_env[e]}")
        loc[e] = got
        for i, c, _ in egos:
            ego_env.append(e); ego_i.append(i); ego_cls.append(c)
    heading = _headings(rng, E, S)
    speed = rng.uniform(1.0, 3.0, (E, n))
    vel = np.stack([speed * np.cos(heading[:, :n]), speed * np.sin(heading[:, :n])], -1)
    ego_env, ego_i = np.array(ego_env), np.array(ego_i)
    return dict(loc=loc, vel=vel, heading=heading, ego_env=ego_env, ego_i=ego_i, ego_cls=np.array(ego_cls),
                ego_wave=wave[ego_env, ego_i], ego_lane=lane[ego_env, ego_i], plan=plan, W=W, epw=epw, n=n, bodies=bodies,
                sq_sense=sq_limit_lt(d_sense), sq_env=sq_env, d_sense=float(d_sense), d_env=d_env, slots=slots,
                poly_envs=np.array([e for e in range(E) if e // epw == poly_group], np.int64))


PLAN_COUNTS = {"zero": 0, "first": 1, "last": 1, "pair": 2, "six": 6, "seven": 7}


def check_plan(b):
    """The model's tied lanes of every wavefront against the plan; returns the counts."""
    n, E = b["n"], b["loc"].shape[0]
    cnt = tied_lanes_per_wave(b["loc"], n, b["d_env"], b["W"], b["epw"])
    act = active_lanes_per_wave(E, n, b["W"], b["epw"])
    nl = sum(1 for j in b["slots"] if j < n)
    for w, kind in b["plan"].items():
        if kind == "all":
            want = act[w] * nl // n
        elif kind == "idle":
            want = 0
        elif kind.startswith("tied"):
            want = int(kind[4:])
        else:
            want = PLAN_COUNTS[kind]
        assert cnt[w] == want, (w, kind, int(cnt[w]), want)
    return cnt

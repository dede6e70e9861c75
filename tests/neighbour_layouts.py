"""Crafted neighbour layouts for the 2-5 UAV kernels, and a host model of their float32 neighbour arithmetic (numpy only).

The library is built with -ffp-contract=off, so numpy float32 reproduces the device's neighbour arithmetic exactly:
  dx = f32(xj - xi), s = f32(f32(dx*dx) + f32(dy*dy)); in range iff s < sq_sense, where sq_sense is the smallest float32 s
  with sqrtf(s) >= f32(d_sense) (sq_limit_lt in uavx_multi_handle.hpp); the distance is the correctly rounded sqrtf(s); the two
  nearest are ordered by (distance, index).
The squared-distance scan of the one-step kernel at N = 4 (scan_neighbours_sq) keeps the three smallest in-range squares
s1 <= s2 <= s3 and sends its whole wavefront through the exact scan when any active lane has s3 < inf and
bits(s3) - bits(s2) <= 8.  A wavefront holds 64 // N whole envs (16 at N = 4): env e sits in wavefront e // (64 // N).

make_batch() builds, for one agent count and sensing range, a deterministic batch of envs whose ego agent sees one of these
neighbour classes (other agents of the env are placed by the same rules, but only the ego is crafted):
  A   exact square ties among the nearest two (A3: among the nearest three), indices shuffled
  B   equal roots from different squares among the nearest two, the lower index on the larger square (the fast-path swap)
  C   equal roots of the 2nd and 3rd by square, the 3rd by square holding the lower index (only the exact order gets it)
  D   s3 - s2 of 1 to 8 ulps with different roots (the fallback is taken)
  E   s3 - s2 of 9 to 64 ulps (the fast path, just past the threshold)
  F   squares at sq_sense - 1 ulp, sq_sense, sq_sense + 1 ulp (F2: two neighbours tied there)
  G   one neighbour (G1) or none (G0) in range
Every agent gets a distinct velocity heading, so a wrong neighbour moves observation columns 6 / 9 by at least 2 / N.
At N = 4 the envs are laid out in 16-env wavefront blocks: "fast" blocks of A / B / E / F / G envs in which no lane is a near
tie, and "fallback" blocks where a single C, D or A3 env pulls the whole wavefront into the exact scan; the last block is
ragged.
"""
import math

import numpy as np

F32 = np.float32
WAVE = 64
INF_BITS = 0x7F800000
FAST_CLASSES = ("A", "B", "E", "F-1", "F0", "F+1", "F2", "G0", "G1")
FALLBACK_CLASSES = ("C", "D", "A3")


def bits(x):
    return np.asarray(x, dtype=F32).view(np.uint32).astype(np.int64)


def sq_limit_lt(lim):
    """Smallest float32 s with sqrtf(s) >= f32(lim): sqrtf(s) < lim  <=>  s < sq_limit_lt(lim)."""
    lim = F32(lim)
    s = F32(lim * lim)
    while s > 0 and np.sqrt(s) >= lim:
        s = np.nextafter(s, F32(0))
    while np.sqrt(s) < lim:
        s = np.nextafter(s, F32(np.inf))
    return F32(s)


def squares(p, q):
    """f32(f32(dx*dx) + f32(dy*dy)) of q - p, float32 throughout (no FMA): p, q [..., 2] float32."""
    p, q = np.asarray(p, F32), np.asarray(q, F32)
    dx = q[..., 0] - p[..., 0]
    dy = q[..., 1] - p[..., 1]
    return dx * dx + dy * dy


def in_range_sorted(loc_env, i, sq_sense):
    """(s, j) of agent i's in-range neighbours, ordered by (s, j)."""
    n = loc_env.shape[0]
    s = squares(loc_env[i], loc_env)
    return sorted((F32(s[j]), j) for j in range(n) if j != i and s[j] < sq_sense)


def nearest_two(loc_env, i, sq_sense):
    """[(j, d), ...] of at most two neighbours, ascending by (float32 distance, index): the reference's order (AG:52-62)."""
    keyed = sorted((F32(np.sqrt(s)), j) for s, j in in_range_sorted(loc_env, i, sq_sense))
    return [(j, d) for d, j in keyed[:2]]


def lane_near_tie(loc_env, i, sq_sense):
    """scan_neighbours_sq's fallback predicate of one active lane: s3 < inf and bits(s3) - bits(s2) <= 8."""
    srt = in_range_sorted(loc_env, i, sq_sense)
    if len(srt) < 3:
        return False
    return int(bits(srt[2][0]) - bits(srt[1][0])) <= 8


def env_near_tie(loc_env, sq_sense):
    return any(lane_near_tie(loc_env, i, sq_sense) for i in range(loc_env.shape[0]))


def wave_fallback(loc, sq_sense):
    """[W] bool: wavefront w of the one-step N = 4 kernel takes the exact scan (lanes past the last env are inactive)."""
    E, n = loc.shape[:2]
    epw = WAVE // n
    env_tie = np.array([env_near_tie(loc[e], sq_sense) for e in range(E)])
    W = (E + epw - 1) // epw
    return np.array([env_tie[w * epw:(w + 1) * epw].any() for w in range(W)])


def classify(loc_env, i, sq_sense):
    """The set of class tags agent i's neighbourhood belongs to (see the module docstring)."""
    srt = in_range_sorted(loc_env, i, sq_sense)
    c = len(srt)
    tags = set()
    if c == 0:
        tags.add("G0")
    if c == 1:
        tags.add("G1")
    sb = [int(bits(s)) for s, _ in srt]
    rt = [F32(np.sqrt(s)) for s, _ in srt]
    if c >= 2 and sb[0] == sb[1]:
        tags.add("A")
    if c >= 3 and sb[0] == sb[1] == sb[2]:
        tags.add("A3")
    if c >= 2 and sb[0] < sb[1] and rt[0] == rt[1] and srt[0][1] > srt[1][1]:
        tags.add("B")
    if c >= 3 and sb[1] < sb[2] and rt[1] == rt[2] and srt[2][1] < srt[1][1]:
        tags.add("C")
    if c >= 3 and 1 <= sb[2] - sb[1] <= 8 and rt[1] != rt[2]:
        tags.add("D")
    if c >= 3 and 9 <= sb[2] - sb[1] <= 64:
        tags.add("E")
    s_all = squares(loc_env[i], loc_env)
    at_edge = {}
    for j in range(loc_env.shape[0]):
        if j != i:
            off = int(bits(s_all[j]) - bits(sq_sense))
            if -1 <= off <= 1:
                tags.add(f"F{off:+d}" if off else "F0")
                at_edge[off] = at_edge.get(off, 0) + 1
    if any(k >= 2 for k in at_edge.values()):
        tags.add("F2")
    return tags


def classes_possible(n):
    """Classes an ego agent with n - 1 neighbours can be in."""
    out = ["F-1", "F0", "F+1", "G0", "G1"]
    if n >= 3:
        out += ["A", "B", "F2"]
    if n >= 4:
        out += ["A3", "C", "D", "E"]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# generator
def _grid(p, ang, r, pred, rng, K=40):
    """A float32 point q near p + r (cos ang, sin ang), within K ulps per axis, whose square to p satisfies pred (or None)."""
    c = (p.astype(np.float64) + r * np.array([math.cos(ang), math.sin(ang)])).astype(F32)
    k = np.arange(-K, K + 1, dtype=np.float64)
    qx = (np.float64(c[0]) + k * np.float64(np.spacing(c[0]))).astype(F32)
    qy = (np.float64(c[1]) + k * np.float64(np.spacing(c[1]))).astype(F32)
    QX, QY = np.meshgrid(qx, qy, indexing="ij")
    q = np.stack([QX.ravel(), QY.ravel()], -1)
    ok = np.flatnonzero(pred(squares(p, q)))
    if ok.size == 0:
        return None
    return q[ok[rng.integers(ok.size)]]


def _point(p, ang, r):
    return (p.astype(np.float64) + r * np.array([math.cos(ang), math.sin(ang)])).astype(F32)


def _craft(rng, cls, n, d_sense, sq):
    """One env of n agents whose ego (returned index) is in class cls, or None if this draw did not reach it."""
    ego = int(rng.integers(n))
    others = [j for j in range(n) if j != ego]
    rng.shuffle(others)
    p = rng.uniform(-8, 8, 2).astype(F32)
    loc = np.zeros((n, 2), F32)
    loc[ego] = p
    a0 = rng.uniform(-math.pi, math.pi)
    step = 2 * math.pi / (n - 1)
    angs = [a0 + k * step + rng.uniform(-0.15, 0.15) * step for k in range(n - 1)]
    r = float(rng.uniform(0.4, 0.75)) * d_sense
    placed = {}   # position in `others` order -> point

    def far(k):   # well out of range
        return _point(p, angs[k], d_sense * rng.uniform(1.3, 1.6))

    def inside(k, frac):   # clearly in range, its square far from the others'
        return _point(p, angs[k], r * frac)

    s_of = lambda q: F32(squares(p, q))
    if cls in ("A", "A3", "B", "C", "D", "E"):
        k0 = 0
        if cls in ("C", "D", "E"):
            placed[0] = inside(0, rng.uniform(0.45, 0.6))
            k0 = 1
        q1 = _point(p, angs[k0], r)
        placed[k0] = q1
        s1 = s_of(q1)
        b1 = int(bits(s1))
        if cls in ("A", "A3"):
            pred = lambda s: bits(s) == b1
        elif cls in ("B", "C"):
            pred = lambda s: (bits(s) > b1) & (np.sqrt(s) == np.sqrt(s1))
        elif cls == "D":
            pred = lambda s: (bits(s) - b1 >= 1) & (bits(s) - b1 <= 8) & (np.sqrt(s) != np.sqrt(s1))
        else:
            lo = int(rng.integers(9, 40))
            pred = lambda s: (bits(s) - b1 >= lo) & (bits(s) - b1 <= 64)
        q2 = _grid(p, angs[k0 + 1], r, pred, rng)
        if q2 is None:
            return None
        placed[k0 + 1] = q2
        if cls == "A3":
            q3 = _grid(p, angs[2], r, pred, rng)
            if q3 is None:
                return None
            placed[2] = q3
    elif cls in ("F-1", "F0", "F+1", "F2"):
        off = {"F-1": -1, "F0": 0, "F+1": 1}.get(cls, int(rng.integers(-1, 2)))
        tb = int(bits(sq)) + off
        pred = lambda s: bits(s) == tb
        q1 = _grid(p, angs[0], d_sense, pred, rng)
        if q1 is None:
            return None
        placed[0] = q1
        if cls == "F2":
            q2 = _grid(p, angs[1], d_sense, pred, rng)
            if q2 is None:
                return None
            placed[1] = q2
        elif n >= 3 and rng.random() < 0.7:
            placed[1] = inside(1, rng.uniform(0.5, 0.9))
    elif cls == "G1":
        placed[0] = inside(0, rng.uniform(0.3, 1.2))
    elif cls != "G0":
        raise ValueError(cls)
    for k in range(n - 1):
        loc[others[k]] = placed[k] if k in placed else far(k)
    if cls in ("B", "C"):
        # the lower index goes to the larger square of the equal-root pair
        k_small, k_big = (0, 1) if cls == "B" else (1, 2)
        a, b = sorted((others[k_small], others[k_big]))
        loc[[b, a]] = loc[[others[k_small], others[k_big]]]
    if cls not in classify(loc, ego, sq):
        return None
    return loc, ego


def _craft_env(rng, cls, n, d_sense, sq, fast):
    """Retries _craft until the class is reached (and, for an env of a fast block at N = 4, no lane is a near tie)."""
    for _ in range(200):
        got = _craft(rng, cls, n, d_sense, sq)
        if got is None:
            continue
        if fast and env_near_tie(got[0], sq):
            continue
        return got
    raise RuntimeError(f"could not craft class {cls} at n={n}, d_sense={d_sense}")


def _plan(rng, n):
    """Class of every env, in batch order."""
    poss = classes_possible(n)
    if n != 4:
        plan = [c for c in poss for _ in range(10)] + poss[:3]   # 53 / 83 / 123 envs: the last wavefront is ragged
        rng.shuffle(plan)
        return plan, None
    pure = [c for c in ("A", "B", "E", "G0", "G1")]
    fast = [c for c in FAST_CLASSES]
    blocks, kinds = [], []
    for _ in range(3):   # fast blocks of A / B / E / G lanes only
        blocks.append([pure[k % len(pure)] for k in rng.permutation(16)])
        kinds.append("fast")
    for _ in range(3):   # fast blocks with the boundary classes
        blocks.append([fast[k % len(fast)] for k in rng.permutation(16)])
        kinds.append("fast")
    for trigger in ("C", "C", "D", "D", "A3"):   # one C / D / A3 env pulls its wavefront into the exact scan
        b = [fast[k % len(fast)] for k in rng.permutation(15)]
        b.insert(int(rng.integers(16)), trigger)
        blocks.append(b)
        kinds.append("fallback")
    blocks.append(["B", "C", "A", "E", "F-1", "G1", "D"])   # ragged last wavefront (7 envs)
    kinds.append("fallback")
    return [c for b in blocks for c in b], kinds


def make_batch(n, d_sense, seed=0):
    """Deterministic crafted batch for n in 2..5: dict(loc [E,n,2] f32, vel [E,n,2] f64 (distinct headings), ego [E],
    cls [E] (the class the ego was built for), sq_sense, kinds (N = 4: "fast" / "fallback" per wavefront block, else None))."""
    assert 2 <= n <= 5
    rng = np.random.default_rng([seed, n, int(round(d_sense * 1000))])
    sq = sq_limit_lt(d_sense)
    plan, kinds = _plan(rng, n)
    E = len(plan)
    loc = np.zeros((E, n, 2), F32)
    ego = np.zeros(E, np.int64)
    for e, cls in enumerate(plan):
        fast = n == 4 and cls not in FALLBACK_CLASSES
        loc[e], ego[e] = _craft_env(rng, cls, n, d_sense, sq, fast)
    # distinct headings: agent k points at a0 + 2 pi k / n (+ a little), speed 1..3
    a0 = rng.uniform(-math.pi, math.pi, (E, 1)) + 2 * math.pi * np.arange(n)[None] / n + rng.uniform(-0.05, 0.05, (E, n))
    speed = rng.uniform(1.0, 3.0, (E, n))
    vel = np.stack([speed * np.cos(a0), speed * np.sin(a0)], -1)
    return dict(loc=loc, vel=vel, ego=ego, cls=np.array(plan), sq_sense=sq, kinds=kinds, d_sense=float(d_sense))


def natural_prev_d(loc, tgt):
    """float32 |tgt - loc| as the device derives prev_distance (no override needed)."""
    return np.sqrt(squares(loc, tgt))


# ---------------------------------------------------------------------------------------------------------------------------
# float64-position layouts (nearest_two64: d = sqrt(fma(dy, dy, dx*dx)) in double, in range iff d < d_sense)
def nrm64(dx, dy):
    """sqrt(fma(dy, dy, dx*dx)) with the single rounding of the fma done exactly (fractions)."""
    from fractions import Fraction
    return math.sqrt(float(Fraction(dy) ** 2 + Fraction(dx * dx)))


def make_batch64(n, d_sense, seed=0):
    """float64 positions for n in 3..5: per env the ego at a point of a 1/64 grid and
      "A64": two (three) neighbours at mirrored offsets of one exact-square offset (exact distance ties), or
      "F64": one or two neighbours (mirrored, tied) at float64 distance prev(d_sense), d_sense or next(d_sense);
    the remaining agents out of range.  Offsets are exactly representable, so the kernel's q - p is the offset itself."""
    rng = np.random.default_rng([seed, n, int(round(d_sense * 1000)), 64])
    E = 48
    loc = np.zeros((E, n, 2), np.float64)
    cls, ego = [], np.zeros(E, np.int64)
    for e in range(E):
        i = int(rng.integers(n))
        others = [j for j in range(n) if j != i]
        rng.shuffle(others)
        p = rng.integers(0, 256, 2) / 64.0 if e % 2 == 0 else np.zeros(2)   # F64: offsets are the positions themselves
        loc[e, i] = p
        if e % 2 == 0:
            dx, dy = [(3.0, 4.0), (5.0, 12.0), (0.75, 1.0), (2.5, 6.0)][e // 2 % 4]
            sc = 0.4 * d_sense / math.hypot(dx, dy)
            sc = 2.0 ** math.floor(math.log2(sc))
            dx, dy = dx * sc, dy * sc
            offs = [(dx, dy), (-dy, dx), (-dx, -dy)][:min(3, n - 1)]
            cls.append("A64")
        else:
            target = [np.nextafter(d_sense, 0.0), d_sense, np.nextafter(d_sense, np.inf)][e // 2 % 3]
            dy = round(0.8 * d_sense * 64) / 64.0
            base = math.sqrt(max(d_sense * d_sense - dy * dy, 0.0))
            ulp = np.spacing(base)
            dx = None
            for m in range(16):   # not every double next to d_sense is a root for one dy: nudge dy too
                dy_m = dy + m * np.spacing(dy)
                for k in range(0, 400):
                    for sgn in (1, -1):
                        c = base + sgn * k * ulp
                        if nrm64(c, dy_m) == target:
                            dx = c
                            break
                    if dx is not None:
                        break
                if dx is not None:
                    dy = dy_m
                    break
            assert dx is not None, (d_sense, target)
            offs = [(dx, dy), (-dx, dy)][:1 + (e // 6) % 2]
            cls.append("F64")
        for k, j in enumerate(others):
            if k < len(offs):
                loc[e, j] = p + np.array(offs[k])
            else:
                a = 2 * math.pi * k / n + 0.3
                loc[e, j] = p + 1.5 * d_sense * np.array([math.cos(a), math.sin(a)])
        ego[e] = i
    a0 = rng.uniform(-math.pi, math.pi, (E, 1)) + 2 * math.pi * np.arange(n)[None] / n
    vel = np.stack([2 * np.cos(a0), 2 * np.sin(a0)], -1)
    return dict(loc=loc, vel=vel, ego=ego, cls=np.array(cls), d_sense=float(d_sense))

"""Crafted layouts that put one agent exactly on, one float step below and one above every comparison of the step kernels that
ends an episode or sets the -2 / +10 rewards, and a host model of those comparisons (numpy only).  Beside neighbour_layouts.py
and key_scan_layouts.py, whose float32 arithmetic (squares, sq_limit_lt) and wavefront models (wave_fallback,
tied_lanes_per_wave, lane_table) are reused.

The library is built with -ffp-contract=off, so plain numpy float32 reproduces the device's float32 arithmetic.  Host model:
  s            = f32(f32(dx*dx) + f32(dy*dy))                      neighbour_layouts.squares
  soft / hard  s <= sq_limit_le(f32(2R)) / s <= sq_limit_le(1)     largest float32 s with sqrtf(s) <= lim (it is NOT lim*lim)
  in range     s <  sq_limit_lt(f32(d_sense))                      smallest float32 s with sqrtf(s) >= lim
  goal         sqrtf(s(target, position)) < 0.5
  speed        fma(vy, vy, vx*vx) < sq_threshold(0.2)              float64, one rounding (done exactly with fractions here)
  box          lo32 <= x <= hi32, lo32 = f32_at_or_above(-size/2), hi32 = f32_at_or_below(size/2)
  move         v' = clip(v + clip((a - v)/tau, +-amax) tau, +-vmax), x' = f32(f64(x) + v' tau); used only with a == v (dv is
               exactly 0: no division) or with a command far past the acceleration clip (dv is exactly +-amax)

make_threshold_batch(n, world) returns a deterministic batch (seeded search) for one of the WORLDS.  A CLASS is a group of member
envs that differ in the last bit(s) of one quantity and lie on both sides of one decision; the ego's tag is (cls, member):
  C    soft collision: square to the nearest neighbour at L-1, L, L+1 ulp and at f32(2R)^2, L = sq_limit_le(f32(2R)); v = a = 0
  Ct   the same with further neighbours 3-6 ulps above L, so that the ego itself is a near-tie lane of both scans (n >= 4)
  H    hard collision: the same members around sq_limit_le(1); the batch is stepped twice (counted once, MUW:208)
  CS   a world with d_sense <= 2R: the neighbour at sq_sense - 1 ulp collides, at sq_sense it is out of range and does not
  GS   the neighbour coasts from L+1 to L (and back): an ego below it sees the old position, an ego above it the new one
  G    goal: norm32(target - position) at 0.5 -1 ulp / 0.5 / 0.5 +1 ulp, axis-aligned and diagonal; one member that would finish
       sits inside 2R of a neighbour (no finish, reward -2)
  S    speed: fma(vy,vy,vx*vx) at lim -1 ulp(f64) / lim / lim +1 ulp, one component (below / at / above 0.2) and two
  O    box: x or y at the limit and 1 ulp outside on each side, standing and coasting into the wall
  V    clips ((a - v)/tau at +-amax, v + dv tau at +-vmax, and 1 ulp(f64) beyond): values only, judged by the oracle
Ego and neighbour indices occur in both orders.  The other agents of a crafted env are parked more than d_sense from everyone
with far targets.  commands="f64": velocities and commands are float64 and moving members coast (command == velocity).
commands="f32": every command is a float32 number; coasting members get a float32 velocity found to land on the same position,
and the S members, whose velocities no float32 holds, reach them through the acceleration clip (command 5 m/s away, dv = amax).
For n = 4 and n >= 7 the crafted envs are repeated in three sections: alone, among envs with one tied lane (every fourth env),
and alternating with regular polygons, so that threshold egos sit in wavefronts with 0, 1-6 and >= 7 near-tie lanes (N = 4: in
fast and in fallback wavefronts of scan_neighbours_sq).  The last wavefront is ragged.
"""
import math
from fractions import Fraction

import numpy as np

import key_scan_layouts as kl
import neighbour_layouts as nl
from neighbour_layouts import F32, bits, sq_limit_lt, squares

TAU, AMAX, VMAX = 0.02, 5.0, 10.0
WORLDS = {
    "r03": dict(collider_radius=0.3, d_sense=3.0, x_size=50.0, y_size=50.0),   # f32(2R) > 2R, 2R < 1, float32-exact box
    "r07": dict(collider_radius=0.7, d_sense=1.8, x_size=12.3, y_size=9.7),    # f32(2R) < 2R, 2R > 1, inexact box halves
    "r10": dict(collider_radius=1.0, d_sense=3.0, x_size=50.0, y_size=50.0),   # f32(2R) == 2R
    "cs": dict(collider_radius=1.0, d_sense=1.4, x_size=50.0, y_size=50.0),    # d_sense <= 2R; sq_sense = f32(1.4)^2 - 1 ulp
}
CLASSES = {"r03": ("C", "Ct", "H", "GS", "G", "S", "O", "V"), "r07": ("C", "H", "O"), "r10": ("C", "H"), "cs": ("CS",)}
SOLO = ("G", "S", "O", "V")            # classes that exist with one agent
SECTIONED = (4, 7, 8, 13, 24)


def classes_of(n, world):
    out = [c for c in CLASSES[world] if n >= 2 or c in SOLO]
    return tuple(c for c in out if c != "Ct" or n >= 4)


def nxt(x, k=1):
    """x moved by k steps of its own type's last bit (float32 in, float32 out; float in, float out)."""
    t = F32 if isinstance(x, np.float32) else np.float64
    x = t(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, t(np.inf) if k > 0 else t(-np.inf))
    return x


def sq_limit_le(lim):
    """Largest float32 s with sqrtf(s) <= f32(lim): sqrtf(s) <= lim  <=>  s <= sq_limit_le(lim)."""
    lim = F32(lim)
    s = F32(lim * lim)
    while np.sqrt(s) <= lim:
        s = np.nextafter(s, F32(np.inf))
    while s > 0 and np.sqrt(s) > lim:
        s = np.nextafter(s, F32(0))
    return F32(s)


def f32_at_or_above(b):
    f = F32(b)
    return nxt(f, 1) if float(f) < b else f


def f32_at_or_below(b):
    f = F32(b)
    return nxt(f, -1) if float(f) > b else f


def sq_threshold(lim):
    """Smallest float64 s with sqrt(s) >= lim: sqrt(s) < lim  <=>  s < sq_threshold(lim)."""
    s = lim * lim
    while math.sqrt(s) >= lim:
        s = float(np.nextafter(s, 0.0))
    while math.sqrt(s) < lim:
        s = float(np.nextafter(s, np.inf))
    return s


SPEED_SQ_LIM = sq_threshold(0.2)


def speed_sq(vx, vy):
    """fma(vy, vy, vx*vx) in float64: the product vx*vx rounded, the fma's single rounding done exactly."""
    return float(Fraction(float(vy)) ** 2 + Fraction(float(vx) * float(vx)))


def norm32(p, q):
    return np.sqrt(squares(p, q))


def move_axis(a, v, x):
    """One axis of AG:26-29 for the cases the model admits -> (v', x')."""
    a, v = float(a), float(v)
    if a == v:
        dv = 0.0
    else:
        assert abs(a - v) > 2 * AMAX * TAU, "the model covers coasting and saturated commands only"
        dv = math.copysign(AMAX, a - v)
    v2 = min(max(v + dv * TAU, -VMAX), VMAX)
    return v2, F32(np.float64(F32(x)) + v2 * TAU)


def _w(world):
    return WORLDS[world] if isinstance(world, str) else world


def limits(world):
    w = _w(world)
    two_r = F32(2 * w["collider_radius"])
    return dict(two_r=two_r, sq_two_r=sq_limit_le(two_r), sq_hard=sq_limit_le(F32(1.0)), sq_sense=sq_limit_lt(w["d_sense"]),
                lo=(f32_at_or_above(-w["x_size"] / 2.0), f32_at_or_above(-w["y_size"] / 2.0)),
                hi=(f32_at_or_below(w["x_size"] / 2.0), f32_at_or_below(w["y_size"] / 2.0)))


# ---------------------------------------------------------------------------------------------------------------------------
# searches (seeded; they run when a batch is made, the tests only read the result)
def _lattice(c, K):
    c = np.asarray(c, F32)
    k = np.arange(-K, K + 1, dtype=np.float64)
    qx = (np.float64(c[0]) + k * np.float64(np.spacing(c[0]))).astype(F32)
    qy = (np.float64(c[1]) + k * np.float64(np.spacing(c[1]))).astype(F32)
    QX, QY = np.meshgrid(qx, qy, indexing="ij")
    return np.stack([QX.ravel(), QY.ravel()], -1)


def _find(rng, p, r, pred, K=48, tries=400, ang=None):
    """A float32 point q at about distance r from p with pred(q [M, 2]) true."""
    p = np.asarray(p, F32)
    for _ in range(tries):
        a = rng.uniform(-math.pi, math.pi) if ang is None else ang + rng.uniform(-0.3, 0.3)
        q = _lattice(p.astype(np.float64) + r * np.array([math.cos(a), math.sin(a)]), K)
        ok = np.flatnonzero(pred(q))
        if ok.size:
            return q[ok[rng.integers(ok.size)]]
    raise RuntimeError("threshold search failed")


def _at_square(rng, p, want, ang=None):
    """q with squares(p, q) == want (a float32), bit for bit."""
    wb = int(bits(want))
    return _find(rng, p, math.sqrt(float(want)), lambda q: bits(squares(p, q)) == wb, ang=ang)


def _coast_velocity(x_old, x_new, f32cmd):
    """v with f32(f64(x_old) + v tau) == x_new (a float32 number if f32cmd), or None."""
    v = (float(x_new) - float(x_old)) / TAU
    for k in range(0, 9):
        for sg in (1, -1):
            c = v * (1 + sg * k * 2e-8)
            c = float(F32(c)) if f32cmd else c
            if move_axis(c, c, x_old)[1] == F32(x_new):
                return c
    return None


# ---------------------------------------------------------------------------------------------------------------------------
class _Env:
    """One crafted env under construction: placed agents (slot -> fields); park() fills the other slots."""

    def __init__(self, n, world, rng):
        self.n, self.world, self.w, self.rng = n, world, _w(world), rng
        self.learners = n                      # slots below this are learners (the rest: scripted bodies)
        self.loc, self.vel, self.tgt, self.act, self.init_d = {}, {}, {}, {}, {}
        self.egos = []

    def put(self, slot, loc, vel=(0.0, 0.0), act=None, tgt=None, init_d=None):
        self.loc[slot] = np.asarray(loc, F32)
        self.vel[slot] = np.asarray(vel, np.float64)
        self.act[slot] = np.asarray(vel if act is None else act, np.float64)
        self.tgt[slot] = None if tgt is None else np.asarray(tgt, F32)
        self.init_d[slot] = init_d

    def pair(self, below):
        """(ego slot, neighbour slot) with ego < neighbour iff below; with bodies: (a learner, a body)."""
        if self.learners < self.n:
            return int(self.rng.integers(self.learners)), int(self.rng.integers(self.learners, self.n))
        if self.n == 2:
            i, j = 0, 1
        else:
            i, j = sorted(int(x) for x in self.rng.choice(self.n, 2, replace=False))
        return (i, j) if below else (j, i)

    def free_slots(self):
        return [k for k in range(self.n) if k not in self.loc]

    def origin(self, span=1.5):
        return self.rng.uniform(-span, span, 2).astype(F32)

    def build(self):
        n, w = self.n, self.w
        d = float(w["d_sense"])
        hx, hy = w["x_size"] / 2.0 - 0.3, w["y_size"] / 2.0 - 0.3
        sp = 1.05 * d
        gx = np.arange(-int(hx / sp), int(hx / sp) + 1) * sp
        gy = np.arange(-int(hy / sp), int(hy / sp) + 1) * sp
        cand = np.stack(np.meshgrid(gx, gy, indexing="ij"), -1).reshape(-1, 2)
        cand = cand[self.rng.permutation(len(cand))]
        placed = [self.loc[k].astype(np.float64) for k in self.loc]
        for k in self.free_slots():
            for c in cand:
                if all(math.hypot(*(c - q)) > 1.04 * d for q in placed):
                    self.put(k, c.astype(F32))
                    placed.append(c.astype(F32).astype(np.float64))
                    break
            else:
                raise RuntimeError(f"no room to park agent {k} of {n} in world {self.world}")
        loc = np.stack([self.loc[k] for k in range(n)])
        vel = np.stack([self.vel[k] for k in range(n)])
        act = np.stack([self.act[k] for k in range(n)])
        tgt = np.zeros((n, 2), F32)
        for k in range(n):
            if self.tgt[k] is not None:
                tgt[k] = self.tgt[k]
            else:   # far away and inside the box: the mirror image, or a fixed offset near the centre
                far = -0.8 * loc[k] if float(np.abs(loc[k]).max()) > 1.5 else loc[k] + F32(2.5) * np.where(loc[k] > 0, -1, 1)
                tgt[k] = far.astype(F32)
        prev_d = norm32(loc, tgt)
        init_d = np.array([prev_d[k] if self.init_d[k] is None else self.init_d[k] for k in range(n)], F32)
        return dict(loc=loc, vel=vel, act=act, tgt=tgt, prev_d=prev_d.astype(F32), init_d=init_d, egos=list(self.egos))


def _slot(rng, n, k):
    """Agent of the k-th member of a one-agent class: agent 0 (whose done bit drives auto-reset) for a fixed share of the members
    on either side of every decision, any agent otherwise."""
    return 0 if (k % 3 == 0 or k % 4 == 1) else int(rng.integers(n))


def _members_around(L, extra=None):
    out = [("L-1", nxt(L, -1)), ("L", L), ("L+1", nxt(L, 1))]
    if extra is not None:
        out.append(("2R^2", extra))
    return out


def _craft_collision(n, world, rng, cls, learners=None):
    """C / Ct / H / CS."""
    lim = limits(world)
    envs = []
    if cls in ("C", "Ct"):
        members = _members_around(lim["sq_two_r"], F32(lim["two_r"] * lim["two_r"]))
        collide = lambda s: bool(s <= lim["sq_two_r"])
    elif cls == "H":
        members = _members_around(lim["sq_hard"], F32(1.0))
        collide = lambda s: bool(s <= lim["sq_hard"])
    else:
        sq = lim["sq_sense"]
        assert _w(world)["d_sense"] <= 2 * _w(world)["collider_radius"] and nxt(sq, 1) <= lim["sq_two_r"]
        members = [("sense-1", nxt(sq, -1)), ("sense", sq), ("sense+1", nxt(sq, 1))]
        collide = lambda s: bool(s < sq)
    for name, want in members:
        for below in (True, False):
            env = _Env(n, world, rng)
            env.learners = learners or n
            i, j = env.pair(below)
            p = env.origin()
            ang = rng.uniform(-math.pi, math.pi)
            env.put(i, p)
            env.put(j, _at_square(rng, p, want, ang))
            if cls == "Ct":   # two more neighbours a few ulps above L: the three smallest squares are a near tie for both scans
                for m, up in enumerate((3, 5)):
                    free = env.free_slots()
                    env.put(free[int(rng.integers(len(free)))], _at_square(rng, p, nxt(lim["sq_two_r"], up), ang + 2.1 * (m + 1)))
            env.egos.append(dict(agent=i, cls=cls, member=name + ("/below" if below else "/above"), other=j, want=want,
                                 expect=collide(want)))
            envs.append(env.build())
    return envs


def _craft_gs(n, world, rng, f32cmd):
    lim = limits(world)
    L, L1 = lim["sq_two_r"], nxt(lim["sq_two_r"], 1)
    envs = []
    for name, old, new in (("L+1>L", L1, L), ("L>L+1", L, L1)):
        for below in (True, False):
            for _ in range(400):
                env = _Env(n, world, rng)
                i, j = env.pair(below)
                p = env.origin()
                q_old = _at_square(rng, p, old)
                near = _lattice(q_old, 3)
                ok = np.flatnonzero(bits(squares(p, near)) == int(bits(new)))
                v = None
                if ok.size:
                    q_new = near[ok[rng.integers(ok.size)]]
                    v = [_coast_velocity(q_old[k], q_new[k], f32cmd) for k in range(2)]
                if v is not None and None not in v:
                    break
            else:
                raise RuntimeError("GS search failed")
            env.put(i, p)
            env.put(j, q_old, vel=v)
            seen = old if below else new            # MUW:198: j < i has moved, j > i has not
            env.egos.append(dict(agent=i, cls="GS", member=f"{name}/{'below' if below else 'above'}", other=j, want=seen,
                                 expect=bool(seen <= L), q_new=q_new))
            envs.append(env.build())
    return envs


def _craft_goal(n, world, rng, learners=None):
    h = F32(0.5)
    envs = []
    goals = [("0.5-1", nxt(h, -1)), ("0.5", h), ("0.5+1", nxt(h, 1))]
    k = -1
    for kind in ("axis", "diag", "blocked"):
        for name, want in goals if kind != "blocked" else goals[:1]:
            if kind == "blocked" and n < 2:
                continue
            k += 1
            env = _Env(n, world, rng)
            wb = int(bits(want))
            if kind == "diag":
                p = env.origin()
                a = rng.uniform(0.5, 1.0) * (1 if rng.random() < 0.5 else -1)      # well off both axes
                t = _find(rng, p, 0.5, lambda q: (bits(norm32(p, q)) == wb) & (np.float64(q[:, 0] - p[0]) ** 2 != (q[:, 0] - p[0]) ** 2)
                          & (np.float64(q[:, 1] - p[1]) ** 2 != (q[:, 1] - p[1]) ** 2), ang=a)
            else:   # the offset itself is the distance: ego on the other axis' line through 0
                ax = int(rng.integers(2))
                p = np.zeros(2, F32)
                p[1 - ax] = env.origin()[0]
                t = p.copy()
                t[ax] = want * F32(1 if rng.random() < 0.5 else -1)
            assert int(bits(norm32(p, t))) == wb
            i = _slot(rng, learners or n, k)
            if kind == "blocked":
                env.learners = learners or n
                i, j = env.pair(bool(rng.random() < 0.5))
                two_r = min(float(limits(world)["two_r"]), float(_w(world)["d_sense"]))      # inside 2R and in range
                env.put(j, (p.astype(np.float64) + 0.8 * two_r * np.array([0.6, -0.8])).astype(F32))
            env.put(i, p, tgt=t, init_d=5.0)
            env.egos.append(dict(agent=i, cls="G", member=f"{kind}/{name}", want=want,
                                 expect=bool(want < h) and kind != "blocked", blocked=kind == "blocked"))
            envs.append(env.build())
    return envs


def _speed_members(rng):
    """[(member, vx, vy)]: one component below / at / above 0.2, two components at lim - 1 ulp, lim, lim + 1 ulp."""
    lim = SPEED_SQ_LIM
    out = [("1c/below", nxt(0.2, -1), 0.0), ("1c/at", 0.2, 0.0), ("1c/above", nxt(0.2, 1), 0.0)]
    k = np.arange(-600, 601)
    vx = 0.12 + k * np.spacing(0.12)
    for name, want in (("2c/lim-1", nxt(lim, -1)), ("2c/lim", lim), ("2c/lim+1", nxt(lim, 1))):
        for _ in range(4000):
            x = float(vx[rng.integers(len(vx))])
            y0 = math.sqrt(want - x * x)
            hit = [y for y in (float(nxt(y0, m)) for m in range(-3, 4)) if speed_sq(x, y) == want]
            if hit:
                out.append((name, x, hit[0]))
                break
        else:
            raise RuntimeError("speed search failed")
    return out


def _craft_speed(n, world, rng, f32cmd):
    envs = []
    for k, (name, vx, vy) in enumerate(_speed_members(rng)):
        sx, sy = (1 if rng.random() < 0.5 else -1), (1 if rng.random() < 0.5 else -1)
        v_new = np.array([sx * vx, sy * vy if vy else 0.0])
        if f32cmd:   # through the acceleration clip: v_old + amax tau == v_new, the command 5 m/s further on
            v_old, act = np.zeros(2), np.zeros(2)
            for k in range(2):
                if v_new[k] == 0.0:
                    continue
                sg = math.copysign(1.0, v_new[k])
                c0 = v_new[k] - sg * AMAX * TAU
                hit = [c for c in (float(nxt(c0, m)) for m in range(-8, 9)) if move_axis(sg * 5.0, c, 0.0)[0] == v_new[k]]
                assert hit, name
                v_old[k], act[k] = hit[0], sg * 5.0
        else:
            v_old, act = v_new.copy(), v_new.copy()
        env = _Env(n, world, rng)
        p = env.origin()
        i = _slot(rng, n, k)
        t = (p.astype(np.float64) + np.array([0.2 * sx, 0.15 * sy])).astype(F32)
        env.put(i, p, vel=v_old, act=act, tgt=t, init_d=5.0)
        env.egos.append(dict(agent=i, cls="S", member=name, want=v_new, expect=speed_sq(*v_new) < SPEED_SQ_LIM))
        envs.append(env.build())
    return envs


def _craft_box(n, world, rng, f32cmd, learners=None):
    lim = limits(world)
    w = _w(world)
    if float(F32(w["x_size"] / 2.0)) != w["x_size"] / 2.0:   # the at-or-below / at-or-above limit is not the nearest float32
        assert any(F32(s * w[k] / 2.0) != (lim["hi"] if s > 0 else lim["lo"])[a]
                   for a, k in enumerate(("x_size", "y_size")) for s in (1, -1))
    envs = []
    k = -1
    for ax in (0, 1):
        for side in ("hi", "lo"):
            edge = lim[side][ax]
            for name, x_new in (("in", edge), ("out", nxt(edge, 1 if side == "hi" else -1))):
                for coast in (False, True):
                    env = _Env(n, world, rng)
                    p = env.origin()
                    v = np.zeros(2)
                    if coast:
                        for _ in range(200):
                            x_old = F32(float(x_new) - (1 if side == "hi" else -1) * rng.uniform(0.02, 0.08))
                            c = _coast_velocity(x_old, x_new, f32cmd)
                            if c is not None:
                                break
                        else:
                            raise RuntimeError("box search failed")
                        p[ax], v[ax] = x_old, c
                    else:
                        p[ax] = x_new
                    k += 1
                    i = _slot(rng, learners or n, k)
                    env.put(i, p, vel=v)
                    env.egos.append(dict(agent=i, cls="O", member=f"{'xy'[ax]}-{side}/{name}/{'coast' if coast else 'still'}",
                                         axis=ax, want=x_new, expect=name == "out"))
                    envs.append(env.build())
    return envs


def _craft_clips(n, world, rng, f32cmd):
    envs = []
    for ax in (0, 1):
        for sg in (1.0, -1.0):
            for k in (0, 1):
                for kind in ("acc", "vel"):
                    v, a = np.zeros(2), np.zeros(2)
                    if kind == "acc":
                        a[ax] = sg * float(nxt(AMAX * TAU, k))
                    else:
                        v[ax], a[ax] = sg * float(nxt(VMAX - AMAX * TAU, k)), sg * 20.0
                    if f32cmd:
                        a = a.astype(F32).astype(np.float64)
                    env = _Env(n, world, rng)
                    i = int(rng.integers(n))
                    env.put(i, env.origin(), vel=v, act=a)
                    env.egos.append(dict(agent=i, cls="V", member=f"{kind}/{'xy'[ax]}{'+' if sg > 0 else '-'}/{k}"))
                    envs.append(env.build())
    return envs


def _tie_env(n, world, rng):
    """Agent 0 with three (n = 3: two) neighbours at one exact square, everyone else parked: exactly one near-tie lane."""
    env = _Env(n, world, rng)
    d = WORLDS[world]["d_sense"]
    a = math.floor(0.8 * d * 64) / 64.0
    p = np.round(rng.uniform(-1, 1, 2) * 4) / 4
    for k, off in enumerate([(0, 0), (a, 0), (-a, 0), (0, a)][:min(n, 4)]):
        env.put(k, p + np.array(off))
    return env.build()


def _polygon_env(n, world, rng):
    env = _Env(n, world, rng)
    side = 0.3 * WORLDS[world]["d_sense"]
    R = side / (2 * math.sin(math.pi / n))
    a = rng.uniform(-math.pi, math.pi) + 2 * math.pi * np.arange(n) / n
    for k in range(n):
        env.put(k, R * np.array([math.cos(a[k]), math.sin(a[k])]))
    return env.build()


_cache = {}


def make_threshold_batch(n, world, commands="f64", seed=0):
    """See the module docstring.  Returns dict(loc, tgt, init_d, prev_d [float32], vel, act [float64; act32: the float32
    commands of a commands="f32" batch], egos: list of dict(env, agent, cls, member, expect, ...), n, world, commands, W, epw,
    section [E] (0 alone, 1 among single ties, 2 among polygons), filler [E] bool, reps: how often a section holds every member (a
    small class list is repeated until a section spans three wavefronts))."""
    key = (n, world, commands, seed)
    if key in _cache:
        return _cache[key]
    assert commands in ("f64", "f32")
    f32cmd = commands == "f32"
    rng = np.random.default_rng([seed, n, sorted(WORLDS).index(world), int(f32cmd)])
    crafted = []
    for cls in classes_of(n, world):
        if cls in ("C", "Ct", "H", "CS"):
            crafted += _craft_collision(n, world, rng, cls)
        elif cls == "GS":
            crafted += _craft_gs(n, world, rng, f32cmd)
        elif cls == "G":
            crafted += _craft_goal(n, world, rng)
        elif cls == "S":
            crafted += _craft_speed(n, world, rng, f32cmd)
        elif cls == "O":
            crafted += _craft_box(n, world, rng, f32cmd)
        else:
            crafted += _craft_clips(n, world, rng, f32cmd)
    reps = 1 if n not in SECTIONED else max(1, -(-3 * nl.WAVE // (n * len(crafted))))   # a section spans three wavefronts or more
    crafted = crafted * reps
    envs, section, filler = [], [], []

    def add(env, sec, fill):
        envs.append(env); section.append(sec); filler.append(fill)

    order = rng.permutation(len(crafted))   # section 0: the envs without a tied lane first, the Ct envs behind them
    for k in sorted(order, key=lambda k: crafted[k]["egos"][0]["cls"] == "Ct"):
        add(crafted[k], 0, False)
    if n in SECTIONED:
        for m, k in enumerate(rng.permutation(len(crafted))):
            add(crafted[k], 1, False)
            if m % 3 == 2:
                add(_tie_env(n, world, rng), 1, True)
        if n != 4:
            for k in rng.permutation(len(crafted)):
                add(_polygon_env(n, world, rng), 2, True)
                add(crafted[k], 2, False)
    while (len(envs) * n) % nl.WAVE == 0 or len(envs) < 3:   # a ragged last wavefront
        add(_tie_env(n, world, rng) if n >= 3 else crafted[0], 1, True)
    egos = []
    for e, env in enumerate(envs):
        if not filler[e]:
            egos += [dict(g, env=e, section=section[e]) for g in env["egos"]]
    b = {k: np.stack([env[k] for env in envs]) for k in ("loc", "vel", "act", "tgt", "prev_d", "init_d")}
    W = kl.group_waves(n) if n in kl.GROUP_WAVES else 1
    b.update(egos=egos, n=n, world=world, commands=commands, W=W, epw=kl.envs_per_group(n, W), section=np.array(section),
             filler=np.array(filler), act32=b["act"].astype(F32), reps=reps)
    if f32cmd:
        assert np.array_equal(b["act32"].astype(np.float64), b["act"])
    _cache[key] = b
    return b


def ego_tied_lane_counts(b, W=None):
    """Per ego: the number of near-tie lanes (key scan model) of the wavefront its lane is in, under W wavefronts a workgroup."""
    W = W or b["W"]
    n, E = b["n"], b["loc"].shape[0]
    cnt = kl.tied_lanes_per_wave(b["loc"], n, WORLDS[b["world"]]["d_sense"], W)
    wave, _ = kl.lane_table(E, n, W)
    return np.array([cnt[wave[g["env"], g["agent"]]] for g in b["egos"]])


def ego_lanes(b, W=None):
    W = W or b["W"]
    wave, lane = kl.lane_table(b["loc"].shape[0], b["n"], W)
    return [(int(wave[g["env"], g["agent"]]), int(lane[g["env"], g["agent"]])) for g in b["egos"]]


def describe(b, e, i=None):
    """'env e agent i class member wavefront w lane l' of the crafted ego of env e (or of agent i if it is one)."""
    wave, lane = kl.lane_table(b["loc"].shape[0], b["n"], b["W"], b["epw"])
    for g in b["egos"]:
        if g["env"] == e and (i is None or g["agent"] == i):
            return (f"env {e} agent {g['agent']} class {g['cls']} member {g['member']} wavefront {wave[e, g['agent']]} "
                    f"lane {lane[e, g['agent']]}")
    return f"env {e} agent {i} (not crafted{', filler' if b['filler'][e] else ''}) wavefront {wave[e, i or 0]} lane {lane[e, i or 0]}"


def world_kwargs(world):
    return dict(WORLDS[world], max_speed=VMAX, max_acceleration=AMAX)


def oracle_for(oracle_mod, b, seed=11):
    """The CPU oracle holding the batch's state (reset once with `seed` so that every other field is what a reset leaves)."""
    E, n = b["loc"].shape[:2]
    orc = oracle_mod.OracleMulti(num_envs=E, num_agents=n, nthreads=8, **world_kwargs(b["world"]))
    orc.reset_philox(seed)
    orc.set_state(loc=b["loc"], vel=b["vel"], tgt=b["tgt"], init_d=b["init_d"], prev_d=b["prev_d"])
    return orc


# ---------------------------------------------------------------------------------------------------------------------------
# scripted bodies and curriculum levels: the neighbour of a C / CS / H ego is a body held still, and the envs of one wavefront
# alternate between two levels whose limits answer the other level's members the other way round
LEVELS = [dict(collider_radius=0.3, d_sense=3.0, x_size=50.0, y_size=50.0),      # soft limit 2R = 0.6
          dict(collider_radius=1.0, d_sense=1.4, x_size=12.3, y_size=9.7)]      # soft limit = the sensing range (d_sense <= 2R)
LEVEL_CLASSES = [("C", "H", "G", "O"), ("CS", "H", "G", "O")]


def make_ext_batch(L, B, leveled=True, seed=0):
    """L learners + B bodies.  leveled: env e is built for LEVELS[e % 2]; else every env for LEVELS[0].  dict(loc [E, L + B, 2]
    (learners, then bodies), vel, act [E, L, 2] (zero: everything stands), tgt, init_d, prev_d [E, L], level [E], egos)."""
    key = ("ext", L, B, leveled, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng([seed, 99, L, B, int(leveled)])
    n = L + B
    per_level = []
    for lv, classes in zip(LEVELS, LEVEL_CLASSES):
        envs = []
        for cls in classes:
            if cls in ("C", "CS", "H"):
                envs += _craft_collision(n, lv, rng, cls, learners=L)
            elif cls == "G":
                envs += _craft_goal(n, lv, rng, learners=L)
            else:
                envs += [e for e in _craft_box(n, lv, rng, False, learners=L) if e["egos"][0]["member"].endswith("still")]
        per_level.append(envs)
    if leveled:
        m = max(len(x) for x in per_level)
        order = [per_level[e % 2][(e // 2) % len(per_level[e % 2])] for e in range(2 * m)]
        level = np.arange(2 * m) % 2
    else:
        order, level = per_level[0], np.zeros(len(per_level[0]), np.int64)
    if (len(order) * L) % nl.WAVE == 0:
        order, level = order[:-2], level[:-2]
    b = {k: np.stack([env[k] for env in order]) for k in ("loc", "vel", "act", "tgt", "prev_d", "init_d")}
    for k in ("vel", "act", "tgt", "prev_d", "init_d"):
        b[k] = np.ascontiguousarray(b[k][:, :L])
    assert not b["vel"].any() and np.isfinite(b["loc"]).all()
    egos = [dict(g, env=e, level=int(level[e])) for e, env in enumerate(order) for g in env["egos"]]
    assert all(g["agent"] < L and g.get("other", L) >= L for g in egos)
    b.update(egos=egos, n=L, L=L, B=B, level=level.astype(np.uint8), leveled=leveled, W=1, epw=kl.envs_per_group(L, 1, B),
             filler=np.zeros(len(order), bool))
    _cache[key] = b
    return b


def other_level_disagrees(g):
    """The decision the OTHER level's limits would take on this ego's quantity, where it is the opposite of the own level's."""
    own, oth = limits(LEVELS[g["level"]]), limits(LEVELS[1 - g["level"]])
    if g["cls"] in ("C", "CS"):
        s = g["want"]
        return bool(s < oth["sq_sense"] and s <= oth["sq_two_r"]) != g["expect"]
    if g["cls"] == "O":
        x, ax = g["want"], g["axis"]
        return (not (oth["lo"][ax] <= x <= oth["hi"][ax])) != g["expect"]
    return False


# ---------------------------------------------------------------------------------------------------------------------------
# single-UAV world (UW:137-173): goal (distance < 0.5: done, +1000) and the box, one agent per env, no neighbours
UW_BOXES = {"b100": dict(x_size=100.0, y_size=100.0), "b12": dict(x_size=12.3, y_size=9.7)}


def make_uw_batch(box, commands="f64", fresh=False, seed=0):
    """dict(loc, tgt, init_d, prev_d [float32], vel, act [float64], vel_f32 [E] uint8, egos).  fresh: the state a reset leaves
    (float32 velocity, vel_f32 = 1: with float32 commands the first step's division is a float32 one, UW:142); then, and with
    commands="f32", the coasting velocities are float32 numbers."""
    key = ("uw", box, commands, fresh, seed)
    if key in _cache:
        return _cache[key]
    f32v = fresh or commands == "f32"
    rng = np.random.default_rng([seed, 77, sorted(UW_BOXES).index(box), int(commands == "f32"), int(fresh)])
    w = UW_BOXES[box]
    lo = (f32_at_or_above(-w["x_size"] / 2.0), f32_at_or_above(-w["y_size"] / 2.0))
    hi = (f32_at_or_below(w["x_size"] / 2.0), f32_at_or_below(w["y_size"] / 2.0))
    h = F32(0.5)
    rows, egos = [], []

    def add(loc, vel, tgt, init_d, **tag):
        loc, tgt = np.asarray(loc, F32), np.asarray(tgt, F32)
        rows.append(dict(loc=loc, vel=np.asarray(vel, np.float64), tgt=tgt, prev_d=norm32(loc, tgt),
                         init_d=F32(init_d if init_d else norm32(loc, tgt))))
        egos.append(dict(tag, env=len(rows) - 1, agent=0))

    for kind in ("axis", "diag"):
        for name, want in (("0.5-1", nxt(h, -1)), ("0.5", h), ("0.5+1", nxt(h, 1))):
            wb = int(bits(want))
            if kind == "diag":
                p = rng.uniform(-1.5, 1.5, 2).astype(F32)
                t = _find(rng, p, 0.5, lambda q: bits(norm32(p, q)) == wb, ang=rng.uniform(0.5, 1.0))
            else:
                ax = int(rng.integers(2))
                p = np.zeros(2, F32)
                p[1 - ax] = F32(rng.uniform(-1.5, 1.5))
                t = p.copy()
                t[ax] = want
            add(p, (0.0, 0.0), t, 5.0, cls="G", member=f"{kind}/{name}", want=want, expect=bool(want < h))
    for ax in (0, 1):
        for side in ("hi", "lo"):
            edge = (hi if side == "hi" else lo)[ax]
            for name, x_new in (("in", edge), ("out", nxt(edge, 1 if side == "hi" else -1))):
                for coast in (False, True):
                    p = rng.uniform(-1.5, 1.5, 2).astype(F32)
                    v = np.zeros(2)
                    if coast:
                        for _ in range(200):
                            x_old = F32(float(x_new) - (1 if side == "hi" else -1) * rng.uniform(0.02, 0.08))
                            c = _coast_velocity(x_old, x_new, f32v)
                            if c is not None:
                                break
                        else:
                            raise RuntimeError("box search failed")
                        p[ax], v[ax] = x_old, c
                    else:
                        p[ax] = x_new
                    add(p, v, -0.5 * p, None, cls="O", member=f"{'xy'[ax]}-{side}/{name}/{'coast' if coast else 'still'}",
                        axis=ax, want=x_new, expect=name == "out")
    E = len(rows)
    b = {k: np.stack([r[k] for r in rows]) for k in ("loc", "vel", "tgt", "prev_d", "init_d")}
    b.update(act=b["vel"].copy(), act32=b["vel"].astype(F32), vel_f32=np.full(E, int(fresh), np.uint8), egos=egos, box=box,
             commands=commands, fresh=fresh)
    if f32v:
        assert np.array_equal(b["act32"].astype(np.float64), b["act"])
    _cache[key] = b
    return b


def uw_oracle_for(oracle_mod, b):
    E = b["loc"].shape[0]
    orc = oracle_mod.OracleSingle(num_envs=E, **UW_BOXES[b["box"]])
    orc.reset_philox(5)
    orc.set_state(loc=b["loc"], vel=b["vel"], tgt=b["tgt"], init_d=b["init_d"], prev_d=b["prev_d"], vel_f32=b["vel_f32"])
    return orc


# ---------------------------------------------------------------------------------------------------------------------------
# float64-position episodes (MUW:157-163): the comparands are the Python floats 2R, 1.0, 0.5, 0.2 and the box halves, the
# distance is sqrt(fma(dy, dy, dx*dx)) of the float64 offsets; every member is one float64 step from its neighbour
WORLD64 = dict(collider_radius=0.7, d_sense=15.0, x_size=12.3, y_size=9.7)


def _offset64(rng, target):
    """(dx, dy) with nrm64(dx, dy) == target exactly (neighbour_layouts.nrm64: the fma's single rounding done exactly)."""
    for _ in range(400):
        a = rng.uniform(0.3, 1.2)
        dy = target * math.sin(a)
        base = math.sqrt(max(target * target - dy * dy, 0.0))
        for k in range(0, 200):
            for sg in (1, -1):
                dx = base + sg * k * float(np.spacing(base))
                if nl.nrm64(dx, dy) == target:
                    return dx, dy
    raise RuntimeError("float64 threshold search failed")


def make_threshold_batch64(seed=0):
    """3 agents, float64 positions: dict(loc, tgt, init_d, prev_d, vel, act [float64], egos).  Classes C64 (2R), H64 (1.0), G64
    (0.5), S64 (0.2, the S members) and O64 (box halves 6.15 / 4.85, standing and coasting); members prev / at / next of the
    limit in float64.  Agent 0 of a pair sits at the origin, so the offset is the neighbour's position itself."""
    key = ("f64", seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng([seed, 64])
    n, w = 3, WORLD64
    two_r = 2 * w["collider_radius"]
    rows, egos = [], []
    park = np.array([[-5.0, -4.0], [5.0, 4.0], [-5.0, 4.0]])

    def add(loc, vel, tgt, ego, **tag):
        loc, tgt = np.array(loc, np.float64), np.array(tgt, np.float64)
        d = np.array([nl.nrm64(*(tgt[i] - loc[i])) for i in range(n)])
        init = d.copy()
        init[ego] = max(init[ego], 5.0)
        rows.append(dict(loc=loc, vel=np.array(vel, np.float64), tgt=tgt, prev_d=d, init_d=init))
        egos.append(dict(tag, env=len(rows) - 1, agent=ego))

    def steps(x):
        return [("prev", float(np.nextafter(x, -np.inf))), ("at", x), ("next", float(np.nextafter(x, np.inf)))]

    far = np.array([[3.0, 3.0], [-3.0, -3.0], [3.0, -3.0]])
    zero = np.zeros((n, 2))
    for cls, lim in (("C64", two_r), ("H64", 1.0)):
        for name, want in steps(lim):
            for below in (True, False):
                i, j = (0, 2) if below else (2, 0)
                loc = park.copy()
                loc[i], loc[j] = (0.0, 0.0), _offset64(rng, want)
                add(loc, zero, far, i, cls=cls, member=f"{name}/{'below' if below else 'above'}", other=j, want=want,
                    expect=want <= lim)
    for kind in ("axis", "diag"):
        for name, want in steps(0.5):
            i = int(rng.integers(n))
            loc, tgt = park.copy(), far.copy()
            loc[i] = (0.0, 0.0)
            tgt[i] = (want, 0.0) if kind == "axis" else _offset64(rng, want)
            add(loc, zero, tgt, i, cls="G64", member=f"{kind}/{name}", want=want, expect=want < 0.5)
    for name, vx, vy in _speed_members(rng):
        i = int(rng.integers(n))
        loc, tgt, vel = park.copy(), far.copy(), zero.copy()
        loc[i], vel[i] = (0.25, -0.5), (vx, vy)
        tgt[i] = loc[i] + (0.2, 0.15)
        add(loc, vel, tgt, i, cls="S64", member=name, want=np.array([vx, vy]), expect=speed_sq(vx, vy) < SPEED_SQ_LIM)
    for ax, half in ((0, w["x_size"] / 2.0), (1, w["y_size"] / 2.0)):
        for side, edge in (("hi", half), ("lo", -half)):
            out = float(np.nextafter(edge, math.copysign(np.inf, edge)))
            for name, x_new in (("in", edge), ("out", out)):
                for coast in (False, True):
                    i = int(rng.integers(n))
                    loc, vel = park.copy(), zero.copy()
                    loc[i] = (0.5, -0.25)
                    loc[i, ax] = x_new
                    if coast:
                        for _ in range(4000):
                            v = math.copysign(rng.uniform(1.0, 4.0), edge)
                            x_old = x_new - v * TAU
                            hit = [x for x in (float(nxt(x_old, m)) for m in range(-4, 5)) if x + v * TAU == x_new]
                            if hit:
                                break
                        else:
                            raise RuntimeError("float64 box search failed")
                        loc[i, ax], vel[i, ax] = hit[0], v
                    add(loc, vel, far, i, cls="O64", member=f"{'xy'[ax]}-{side}/{name}/{'coast' if coast else 'still'}", axis=ax,
                        want=x_new, expect=name == "out")
    b = {k: np.stack([r[k] for r in rows]) for k in ("loc", "vel", "tgt", "prev_d", "init_d")}
    b.update(act=b["vel"].copy(), egos=egos, n=n)
    _cache[key] = b
    return b


def oracle_for64(oracle_mod, b, seed=12):
    E, n = b["loc"].shape[:2]
    orc = oracle_mod.OracleMulti(num_envs=E, num_agents=n, nthreads=4, max_speed=VMAX, max_acceleration=AMAX, **WORLD64)
    orc.reset_philox(seed)
    orc.set_state(loc=b["loc"], vel=b["vel"], tgt=b["tgt"], init_d=b["init_d"], prev_d=b["prev_d"])
    orc.f64pos[:] = 1
    return orc


def ext_kwargs(b):
    return dict(num_agents=b["L"], num_bodies=b["B"], body_speed=0.0, body_period=128, body_seed=5, max_speed=VMAX,
                max_acceleration=AMAX, **LEVELS[0])


def body_records(b):
    """[E, B, 6] {x, y, dx, dy, heading, legs} of bodies held still at the batch's positions."""
    rec = np.zeros((b["loc"].shape[0], b["B"], 6), F32)
    rec[..., :2] = b["loc"][:, b["L"]:]
    return rec


def ext_setup(world, b, seed=13):
    """Brings a device batch or an oracle (same method names) into the batch's state: levels, reset, bodies, learners."""
    if b["leveled"]:
        world.set_curriculum(LEVELS)
        world.set_env_levels(b["level"])
    if hasattr(world, "reset_philox"):
        world.reset_philox(seed)
        world.body[...] = body_records(b)
    else:
        world.reset()
        world.set_bodies(body_records(b))
    world.set_state(loc=b["loc"][:, :b["L"]], vel=b["vel"], tgt=b["tgt"], init_d=b["init_d"], prev_d=b["prev_d"])
    return world

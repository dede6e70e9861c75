"""Crowded reset layouts: a numpy restatement of the episode start and the cases that make its accept / reject chain work.

The reference draws start points and targets in a sequential loop (MUW:126-153): agent i keeps the first candidate farther than
2R from the accepted points of the agents j < i; a target must also be clear of the agent's own start.  The device replays that
loop in parallel in three implementations (csrc/uavx_multi_reset.hpp: reset_envs_wave in place, stage_ahead one lane per slot with
an incremental clash bitmap on one wavefront and a full re-test on several), and every other test of the suite draws in boxes so
roomy that a slot almost never needs a third candidate.  This module

  * restates the addressed candidate stream from the text of include/uavx.h and the comments of csrc/uavx_device.hpp (NOT by
    calling the oracle): Philox4x32-10 with counter (env[31:0], env[47:32] | slot << 16, attempt, episode) under the reset seed,
    words 0,1 = the start candidate, words 2,3 = the target candidate, as 32-bit uniforms over the box cast to float32; the
    env's level from pseudo-slot 0xFFFF; a body's waypoint 0 from counter word 2 = 0x80000000 | leg under the body seed;
  * replays the sequential chain in numpy (all envs side by side, slot after slot, attempt after attempt: the order inside an env
    is the reference's) and returns, besides the layout, the number of candidates every slot took and per-env EVENT flags that
    say which corners of the device's bookkeeping the env exercises;
  * holds the table CROWDED of cases and the schedule (seeds, second world, episode indices) the GPU tests run them on.

tests/test_reset_layouts_host.py proves on the CPU that the restatement equals the oracle bit for bit, that no slot of any case,
seed, world and episode used needs more than MAX_ATTEMPTS candidates (so no device loop can run long), and that every event is
present in numbers; tests/test_gpu_reset_crowded.py runs the kernels."""
from collections import namedtuple

import numpy as np

TAU = 0.02                  # MUW:26
FLAG_INACTIVE = 32          # include/uavx.h UAVX_FLAG_INACTIVE: a learner parked by its env's level
LEVEL_SLOT = 0xFFFF         # pseudo-slot whose stream draws the env's level
WAYPOINT = 0x80000000       # counter word 2 of a body's waypoint: 0x80000000 | leg
CHAIN_ROWS = 4              # kChainRows: accepted rows a clash loop of the device reads per trip
MAX_ATTEMPTS = 512          # boundedness condition: no slot of any case may need more candidates than this
EPISODES = 10               # episode indices 0 .. EPISODES - 1: what the GPU tests can reach (16 calls with a step cap of 1
                            # start 8 episodes after the first; an explicit masked reset and a reseeding reset add one each)
BIG_OFFSET = 2 ** 40 + 3    # a global env id with bits 32-47 set: they travel in counter word 1 beside the slot

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays of counters: c0..c3 broadcastable uint32 arrays, key (k0, k1) two ints.
    Returns the four output words as uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & _LO32 for c in (c0, c1, c2, c3)])
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2          # 32 x 32 -> 64 bit products: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO32, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO32
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def reset_words(ge, slot, attempt, episode, seed):
    """The four words of candidate `attempt` of `slot` in global env `ge` for the episode with index `episode`."""
    ge = np.asarray(ge, dtype=np.uint64)
    hi = (ge >> _S32) & np.uint64(0xFFFF)
    slot = np.asarray(slot, dtype=np.uint64)
    return philox4x32_10(ge & _LO32, hi | (slot << np.uint64(16)), attempt, episode, int(seed) & 0xFFFFFFFF, int(seed) >> 32)


def point(x_size, y_size, wx, wy):
    """np.random.uniform(lo, hi, (2,)).astype(float32) with 32-bit uniforms: float32(lo + (hi - lo) * w / 2^32)."""
    lox, loy, hix, hiy = -x_size / 2.0, -y_size / 2.0, x_size / 2.0, y_size / 2.0
    u, v = wx.astype(np.float64) * (1.0 / 4294967296.0), wy.astype(np.float64) * (1.0 / 4294967296.0)
    return (lox + (hix - lox) * u).astype(np.float32), (loy + (hiy - loy) * v).astype(np.float32)


def too_close(two_r, ax, ay, bx, by):
    """The clearance test as the oracle states it: float32(norm) <= float32(2R), norm = sqrt(fl(dx*dx) + fl(dy*dy)) in float32."""
    dx, dy = ax - bx, ay - by
    assert dx.dtype == np.float32
    return np.sqrt(dx * dx + dy * dy) <= two_r


def _fma32(a, b, c):
    """fmaf on float32 arrays, correctly rounded: the product is exact in float64, the sum is rounded to odd there (two-sum), and
    53 >= 2 * 24 + 2 bits make the final rounding to float32 the rounding of the exact value."""
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    away = (err > 0) == (s > 0)
    bits[fix & away] += 1
    bits[fix & ~away] -= 1
    return bits.view(np.float64).astype(np.float32)


def atan2_leg(y, x):
    """Heading of a leg (csrc/uavx_device.hpp atan2_exact: octant reduction, Cephes atanf polynomial, IEEE division)."""
    f = np.float32
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    big = mn > f(0.41421356237) * mx
    num = np.where(big, mn - mx, mn)
    den = np.where(big, mn + mx, mx)
    den = np.where(mx == 0, f(1), den)
    t = (num / den).astype(f)
    z = t * t
    pl = _fma32(np.full_like(z, f(8.05374449538e-2)), z, np.full_like(z, f(-1.38776856032e-1)))
    pl = _fma32(pl, z, np.full_like(z, f(1.99777106478e-1)))
    pl = _fma32(pl, z, np.full_like(z, f(-3.33329491539e-1)))
    r = _fma32(pl * z, t, t)
    r = np.where(big, r + f(0.78539816339744830962), r)
    r = np.where(ay > ax, f(1.57079632679489661923) - r, r)
    r = np.where(x < 0, f(3.14159265358979323846) - r, r)
    return np.copysign(r, y).astype(f)


def body_leg(px, py, wx, wy, body_step):
    """{dx, dy, heading, legs} of a leg from P to waypoint W (include/uavx.h, uavx_set_body_rule): float32, no FMA."""
    f = np.float32
    dx, dy = wx - px, wy - py
    d = np.sqrt(dx * dx + dy * dy)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = f(body_step) / d
        legs = np.floor(d / f(body_step))
    on = d > 0
    return (np.where(on, dx * sc, f(0)).astype(f), np.where(on, dy * sc, f(0)).astype(f), atan2_leg(dy, dx),
            np.where(on, legs, f(0)).astype(f))


class Unbounded(AssertionError):
    pass


EVENTS = ("deep", "deeper", "set_bit", "clear_bit", "body_vs_learner", "own_start", "tail_trip")


def _chain(ge, ep, seed, L, nl, nb, x_size, y_size, radius, cap, pairs=True):
    """The sequential chain for envs that share one world: rows 0 .. nl - 1 are the learners taking part, rows nl .. nl + nb - 1
    the bodies (slots L ..).  Returns start [n, nl + nb, 2], target [n, nl, 2], attempts [n, nl + nb] / [n, nl], events."""
    n, rows = len(ge), nl + nb
    two_r = np.float32(2 * radius)
    slots = list(range(nl)) + [L + b for b in range(nb)]
    ev = {k: np.zeros(n, bool) for k in EVENTS}
    out = []
    for phase, cnt in ((0, rows), (1, nl)):
        acc = np.zeros((n, cnt, 2), np.float32)
        first = np.zeros((n, cnt, 2), np.float32)
        att = np.zeros((n, cnt), np.int32)
        for r in range(cnt):
            pending = np.arange(n)
            k = 0
            while pending.size:
                if k >= cap:
                    raise Unbounded(f"slot {slots[r]} phase {phase}: {pending.size} env(s) past {cap} candidates "
                                    f"(first global env {int(ge[pending[0]])}, episode {int(ep[pending[0]])})")
                # the next K candidates of every env still looking, side by side; an env takes the FIRST of them that is clear
                # and only the ones before it count as drawn (the order inside an env stays the reference's)
                K = min(2 if k == 0 else 8, cap - k)
                w = reset_words(ge[pending, None], slots[r], (k + np.arange(K))[None, :], ep[pending, None], seed)
                px, py = point(x_size, y_size, w[2 * phase], w[2 * phase + 1])                               # [m, K]
                if k == 0:
                    first[:, r, 0], first[:, r, 1] = px[:, 0], py[:, 0]
                C = too_close(two_r, acc[pending, None, :r, 0], acc[pending, None, :r, 1], px[:, :, None], py[:, :, None])   # [m, K, r]
                lower = C.any(axis=2)
                own = np.zeros(lower.shape, bool)
                if phase:
                    own = too_close(two_r, px, py, out[0][0][pending, None, r, 0], out[0][0][pending, None, r, 1])   # MUW:146
                rej = lower | own
                found = ~rej.all(axis=1)
                take = np.where(found, np.argmax(~rej, axis=1), K)            # candidates 0 .. take - 1 of this batch were rejected
                drawn = np.arange(K)[None, :] < take[:, None]
                if phase:
                    ev["own_start"][pending] |= (own & ~lower & drawn).any(axis=1)
                if r % CHAIN_ROWS:      # the last trip of the device's clash loop is a partial one
                    t0 = CHAIN_ROWS * ((r - 1) // CHAIN_ROWS)
                    ev["tail_trip"][pending] |= (C[:, :, t0:].any(axis=2) & ~C[:, :, :t0].any(axis=2) & ~own & drawn).any(axis=1)
                if phase == 0 and r >= nl:
                    ev["body_vs_learner"][pending] |= (C[:, :, :nl].any(axis=2) & drawn).any(axis=1)
                ok, at = pending[found], take[found]
                acc[ok, r, 0], acc[ok, r, 1] = px[found, at], py[found, at]
                att[ok, r] = k + at + 1
                pending = pending[~found]
                k += K
        ev["deep"] |= (att >= 3).any(axis=1)
        ev["deeper"] |= (att >= 5).any(axis=1)
        out.append((acc, att))
        if not pairs:
            continue
        # what the incremental clash bitmap of stage_ahead has to follow: slot j > i against i's FIRST and ACCEPTED candidate
        a = too_close(two_r, first[:, :, None, 0], first[:, :, None, 1], first[:, None, :, 0], first[:, None, :, 1])   # [n, j, i]
        b = too_close(two_r, first[:, :, None, 0], first[:, :, None, 1], acc[:, None, :, 0], acc[:, None, :, 1])
        below = np.tril(np.ones((cnt, cnt), bool), -1)[None]
        ev["set_bit"] |= (~a & b & below).any(axis=(1, 2))
        ev["clear_bit"] |= (a & ~b & below & (att == 1)[:, :, None]).any(axis=(1, 2))
    return out[0][0], out[1][0], out[0][1], out[1][1], ev


def draw_levels(world, ge, ep, seed):
    """The level every env takes at this reset: uniform in the window from word 0 of pseudo-slot 0xFFFF (random window only)."""
    levels, (lo, hi) = world["levels"], world["window"]
    if not levels:
        return np.zeros(len(ge), np.uint8)
    assert lo >= 0, "the crowded cases use the random window"
    w0 = reset_words(ge, LEVEL_SLOT, 0, ep, seed)[0].astype(np.uint64)
    lvl = lo + ((w0 * np.uint64(hi - lo + 1)) >> _S32).astype(np.int64)
    return np.minimum(lvl, len(levels) - 1).astype(np.uint8)


def draw_layouts(case, world, seed, episode, cap=MAX_ATTEMPTS, envs=None, pairs=True):
    """Layouts of the envs of `case` (all, or the local indices `envs`) in `world` (one of worlds(case)) for the episode with
    index `episode` (an int or one per env).  Returns a dict: loc, tgt [E, L, 2] and init_d [E, L] float32, flags [E, L] uint8,
    body [E, B, 6] float32, level [E] uint8, attempts [E, L + B, 2] (candidates taken per slot: starts / targets; 0 = takes no
    part) and one bool [E] per name in EVENTS (pairs=False leaves out set_bit and clear_bit, which cost a test per pair of slots)."""
    idx = np.arange(case.E) if envs is None else np.asarray(envs)
    n, L, B = len(idx), case.L, case.B
    ge = (np.uint64(case.env_offset) + idx.astype(np.uint64))
    ep = np.broadcast_to(np.asarray(episode, dtype=np.uint32), (n,)).copy()
    level = draw_levels(world, ge, ep, seed)
    res = dict(loc=np.full((n, L, 2), np.inf, np.float32), tgt=np.zeros((n, L, 2), np.float32),
               init_d=np.full((n, L), np.inf, np.float32), flags=np.full((n, L), FLAG_INACTIVE, np.uint8),
               body=np.zeros((n, B, 6), np.float32), level=level, attempts=np.zeros((n, L + B, 2), np.int32))
    res["body"][:, :, :2] = np.inf
    for k in EVENTS:
        res[k] = np.zeros(n, bool)
    table = world["levels"] or [dict(x_size=world["x_size"], y_size=world["y_size"], collider_radius=world["collider_radius"])]
    for lv, spec in enumerate(table):
        sel = np.flatnonzero(level == lv)
        if not sel.size:
            continue
        nl = min(max(int(spec.get("n_active", L)), 1), L)
        nb = min(max(int(spec.get("b_active", B)), 0), B)
        xs, ys = float(spec["x_size"]), float(spec["y_size"])
        start, target, att_s, att_t, ev = _chain(ge[sel], ep[sel], seed, L, nl, nb, xs, ys, float(spec["collider_radius"]), cap, pairs)
        res["loc"][sel, :nl] = start[:, :nl]
        res["tgt"][sel, :nl] = target
        d = target - start[:, :nl]
        res["init_d"][sel, :nl] = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])                # MUW:154
        res["flags"][sel, :nl] = 0
        res["attempts"][sel, :nl, 0] = att_s[:, :nl]
        res["attempts"][sel, :nl, 1] = att_t
        if nb:
            res["attempts"][sel, L:L + nb, 0] = att_s[:, nl:]
            slot = (L + np.arange(nb))[None, :]
            hi = (ge[sel] >> _S32) & np.uint64(0xFFFF)
            bs = case.body_seed
            w = philox4x32_10((ge[sel] & _LO32)[:, None], hi[:, None] | (slot.astype(np.uint64) << np.uint64(16)), WAYPOINT | 0,
                              (ep[sel] & np.uint32(0x7FFFFFFF))[:, None], bs & 0xFFFFFFFF, bs >> 32)
            wx, wy = point(xs, ys, w[0], w[1])
            px, py = start[:, nl:, 0], start[:, nl:, 1]
            dx, dy, heading, legs = body_leg(px, py, wx, wy, np.float32(case.body_speed * TAU))
            res["body"][sel, :nb] = np.stack([px, py, dx, dy, heading, legs], axis=-1)
        for k in EVENTS:
            res[k][sel] = ev[k]
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# The cases.  Boxes and radii: a plain-uniform simulation of the chain (200 envs per case) gave 1.9 - 5 candidates per slot on
# average and maxima of 16 - 140 for these; boxes nearer the jamming limit (24 + 40 or 8 + 16 slots at 0.9 per unit area) ran
# into the thousands and are not used.  E is 500 - 1100 and mostly no multiple of 64 (a partial last wavefront / workgroup).
Case = namedtuple("Case", "name L B x_size y_size radius levels window window2 box2 E seed seed2 env_offset d_sense "
                          "body_speed body_period body_seed")


def _case(name, L, B, x, y, r, E, seed, env_offset=11, box2=None, levels=None, window=(-1, -1), window2=None):
    return Case(name, L, B, float(x), float(y), float(r), levels, window, window2, box2, E, seed, seed + 1000, env_offset,
                d_sense=4.0, body_speed=3.0, body_period=4, body_seed=77 + L)


# one level with a single learner and no body (no chain at all) beside jammed ones: a chain-free env shares its wavefront with
# envs that redraw many times; the levels differ in box, radius and in how many learners / bodies take part
CURRICULUM = [dict(x_size=9.0, y_size=9.0, collider_radius=0.5, d_sense=4.0, n_active=1, b_active=0),
              dict(x_size=7.0, y_size=6.5, collider_radius=0.5, d_sense=4.0, n_active=8, b_active=16),
              dict(x_size=5.5, y_size=4.5, collider_radius=0.6, d_sense=3.0, n_active=5, b_active=3),
              dict(x_size=8.0, y_size=7.0, collider_radius=0.75, d_sense=5.0, n_active=3, b_active=9)]

CROWDED = [
    _case("2", 2, 0, 3.4, 3.4, 1.0, 1000, 101, box2=(3.6, 3.3)),
    _case("4", 4, 0, 6, 6, 1.0, 1027, 102, box2=(6.0, 5.5)),
    _case("5", 5, 0, 7, 5, 1.0, 901, 103, env_offset=BIG_OFFSET, box2=(6.5, 5.5)),
    _case("8", 8, 0, 8, 8, 1.0, 1024, 104, box2=(8.5, 7.5)),
    _case("13", 13, 0, 8, 8, 0.75, 777, 105, box2=(8.5, 7.5)),
    _case("24", 24, 0, 10, 10, 0.6, 650, 106, env_offset=BIG_OFFSET, box2=(10.5, 9.5)),
    _case("64", 64, 0, 14, 14, 0.5, 500, 107, box2=(14.5, 13.5)),
    _case("3+5", 3, 5, 4, 4, 0.5, 1100, 108, box2=(4.2, 3.8)),
    _case("8+16", 8, 16, 7, 6, 0.5, 1000, 109, env_offset=BIG_OFFSET, box2=(6.5, 6.5)),
    _case("24+40", 24, 40, 14, 14, 0.5, 515, 110, box2=(14.5, 13.5)),
    _case("levels", 8, 16, 9, 9, 0.5, 1000, 111, env_offset=BIG_OFFSET, levels=CURRICULUM, window=(0, 3), window2=(1, 2)),
]
BY_NAME = {c.name: c for c in CROWDED}
CHAIN_FREE_LEVEL = 0


def env_kwargs(case):
    """Constructor keywords shared by BatchedMultiUAVWorld2D and OracleMulti."""
    kw = dict(num_agents=case.L, x_size=case.x_size, y_size=case.y_size, collider_radius=case.radius, d_sense=case.d_sense)
    if case.B:
        kw.update(num_bodies=case.B, body_speed=case.body_speed, body_period=case.body_period, body_seed=case.body_seed)
    return kw


def worlds(case):
    """The two worlds a case is run in: as created, and after the change in the middle of the staged run (set_config to another
    crowded box; with a curriculum, where the world is the level table, the level window moves instead)."""
    first = dict(x_size=case.x_size, y_size=case.y_size, collider_radius=case.radius, levels=case.levels, window=case.window)
    second = dict(first)
    if case.levels:
        second["window"] = case.window2
    else:
        second["x_size"], second["y_size"] = case.box2
    return first, second


def envs_per_wave(case):
    """Consecutive envs that share a wavefront of the in-place chain (one lane per learner; with bodies or levels the LDS rows
    of the extension kernels bound it as well)."""
    ext = 192 // (case.L + case.B) if (case.B or case.levels) else 64
    return max(1, min(64 // case.L, ext))

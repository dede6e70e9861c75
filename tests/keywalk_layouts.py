"""Crafted replay rings for the n-step walk from keys (include/uavx_keywalk.h), built in numpy: test_keywalk_host.py proves
on the CPU that they hold what the tests need (every stop reason, every length, the ignored kinds of key), and
test_gpu_prio_nstep.py uploads the same arrays.

8 envs x 4 agents.  Observation cells are unique (arange), rewards normal with one column of −0, and the flags go by env,
as tests/test_gpu_nstep.py::_craft has them:
    env 0  every cell a reset row (skip);   env 1  clean;
    env 2  agents 1 and 2 done at steps c − 1 and c − 3;   env 3  ended and truncated at those steps;
    env 4  skip at those steps;   envs 5..  done / skip / ended / trunc at random, rate 0.3."""
import collections

import numpy as np

E, N = 8, 4
HORIZONS = (5, 9)
COUNTS = ("2", "T", "T+1", "2T+3")

Layout = collections.namedtuple("Layout", "T count packed learners obs act rew done skip trunc ended")


def count_of(name, T):
    return {"2": 2, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3}[name]


def craft(T, count, packed, seed=0, learners=N):
    """-> Layout.  done carries the flags in bits 1 / 3 / 2 of agent 0's byte when `packed`; skip, trunc and ended [L, E] are
    the flags themselves in both layouts (a packed ring does not read them)."""
    L = T + 1
    g = np.random.default_rng(1000 * T + 10 * count + seed)
    obs = np.arange(L * E * N * 10, dtype=np.float32).reshape(L, E, N, 10)
    act = (-np.arange(L * E * N * 2, dtype=np.float32) - 1).reshape(L, E, N, 2)
    rew = g.standard_normal((L, E, N)).astype(np.float32)
    rew[:, 1, 3] = -0.0                                     # a return of −0 keeps its sign (the outputs are compared as bits)
    done = (g.random((L, E, N)) < 0.3).astype(np.uint8)
    skip = (g.random((L, E)) < 0.3).astype(np.uint8)
    ended = (g.random((L, E)) < 0.3).astype(np.uint8)
    trunc = ended & (g.random((L, E)) < 0.5).astype(np.uint8)
    done[:, :5], skip[:, :5], ended[:, :5], trunc[:, :5] = 0, 0, 0, 0
    skip[:, 0] = 1
    for step in (count - 1, count - 3):
        if step >= 0:
            s = step % L
            done[s, 2, 1:3], ended[s, 3], trunc[s, 3], skip[s, 4] = 1, 1, 1, 1
    if packed:
        done[:, :, 0] |= skip * 2 + trunc * 8 + ended * 4
    return Layout(T, count, bool(packed), learners, obs, act, rew, done, skip, trunc, ended)


def ring(lay):
    """The ring arguments of keywalk_ref.walk / nstep_ref.sample: a packed ring hands over no flag arrays."""
    kw = dict(obs=lay.obs, rew=lay.rew, done=lay.done)
    if not lay.packed:
        kw.update(skip=lay.skip, trunc=lay.trunc, ended=lay.ended)
    return kw


def window(lay):
    """(c, lo, span, per) of the header."""
    c = max(1, lay.count)
    lo = max(0, c - lay.T)
    return c, lo, c - lo, E * lay.learners


def cell_keys(lay, steps=None, envs=None):
    """The key of every cell of (steps, default the window) x (envs, default all) x learners, step-major."""
    c, lo, span, per = window(lay)
    steps = np.arange(lo, c) if steps is None else np.asarray(list(steps), dtype=np.int64)
    envs = np.arange(E) if envs is None else np.asarray(list(envs), dtype=np.int64)
    k, e, i = np.meshgrid(steps, envs, np.arange(lay.learners), indexing="ij")
    return (k * per + e * lay.learners + i).ravel().astype(np.int64)


def ignored_keys(lay):
    """One key of every ignored kind: −1, −2^63, a cell of step lo − 1 (when there is one), a cell of step c, 2^62."""
    c, lo, span, per = window(lay)
    out = [-1, -2 ** 63]
    if lo > 0:
        out.append((lo - 1) * per + per - 1)
    out += [c * per + 5, 2 ** 62]
    return np.asarray(out, dtype=np.int64)


def keys(lay):
    """Every cell of the window, then the ignored kinds: at most 9·8·4 + 5 rows."""
    return np.concatenate([cell_keys(lay), ignored_keys(lay)])

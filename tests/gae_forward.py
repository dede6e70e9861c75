"""GAE(λ) by its definition, in exact arithmetic: the forward view, for tests/test_gae_host.py.

For a step k of the window and a learner (e, i) whose row is not a re-initialisation row,

    A(k) = Σ_{l ≥ 0} (γλ)^l · δ(k + l)      up to and including the first row k + l that stops,
    δ(k) = r(k) + (done(k) ? 0 : γ·V(k + 1)) − V(k),

where a row k stops on the agent's own done, on the end of its env's episode, when k + 1 is not a step of the ring yet
(k + 1 ≥ count) and when row k + 1 is a re-initialisation row.  Nothing here is a recurrence and nothing is shared with
gae_ref.py: every entry is summed on its own, in fractions.Fraction, from the float32 inputs and the float64 γ and λ.  Next to
each sum goes the same sum with every term replaced by its absolute value, which is what a rounding-error bound scales with."""
from fractions import Fraction


def forward_view(rew, done, values, count, steps, gamma, lam, learners, skip=None, ended=None):
    """{(k, e, i): (A, A + V(k), M, M + |V(k)|)} over the valid entries of the window, as Fractions.  The flags are skip /
    ended arrays [L, E] or, when both are None, bits 1 and 2 of done[:, :, 0]."""
    L, E, N = rew.shape
    g, gl = Fraction(float(gamma)), Fraction(float(gamma)) * Fraction(float(lam))
    F = lambda x: Fraction(float(x))

    def flag(bit, rows, k, e):
        return bool(done[k % L, e, 0] & bit) if rows is None else bool(rows[k % L, e])

    out = {}
    for k in range(count - steps, count):
        for e in range(E):
            if flag(2, skip, k, e):
                continue
            for i in range(learners):
                A = M = Fraction(0)
                w = Fraction(1)
                j = k
                while True:
                    s, s1 = j % L, (j + 1) % L
                    d = bool(done[s, e, i] & 1)
                    A += w * (F(rew[s, e, i]) + (0 if d else g * F(values[s1, e, i])) - F(values[s, e, i]))
                    M += w * (abs(F(rew[s, e, i])) + (0 if d else g * abs(F(values[s1, e, i]))) + abs(F(values[s, e, i])))
                    if d or flag(4, ended, j, e) or j + 1 >= count or flag(2, skip, j + 1, e):
                        break
                    w *= gl
                    j += 1
                V = F(values[k % L, e, i])
                out[(k, e, i)] = (A, A + V, M, M + abs(V))
    return out

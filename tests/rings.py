"""Seeded Dirichlet rings for the boundary tests (numpy only).

A ring g holds 4(N+1) doubles, side-major (include/mgx.h, mgx_set_boundary):
g[0] = u(0, :), g[1] = u(N, :), g[2] = u(:, 0), g[3] = u(:, N).  The four
corners belong to the two row sides.

ring(N, k) is the ring of step k: smooth O(1) data that moves with k plus
N(0, .05) noise, a pure function of (N, k), so that three steps carry three
different rings and a pass that took a ring from a stale buffer shows.
"""
import numpy as np


def ring(N, k):
    """-> (4, N+1) float64: the ring of step k (the rng draws in the order g0,
    g1, g2, g3)."""
    x = np.arange(N + 1) / N
    t = 0.3 * k
    rng = np.random.default_rng(7000 + k)

    def noise():
        return .05 * rng.standard_normal(N + 1)
    g0 = .8 * np.sin(2 * np.pi * x + t) + .2 * (k + 1) + noise()
    g1 = .5 * np.cos(3 * np.pi * x - t) - .1 * k + noise()
    g2 = .6 * np.sin(np.pi * x * (k + 1)) + noise()
    g3 = np.exp(-20 * (x - .2 - .1 * k) ** 2) + noise()
    return np.ascontiguousarray(np.stack([g0, g1, g2, g3]))


def put(u, N, g):
    """Write ring g into the flat (N+1)^2 array u in place: the columns first,
    then the rows, so the rows win at the corners.  Returns u."""
    U = u.reshape(N + 1, N + 1)
    g = np.asarray(g).reshape(4, N + 1)
    U[:, 0] = g[2]
    U[:, N] = g[3]
    U[0, :] = g[0]
    U[N, :] = g[1]
    return u


def get(u, N):
    """The ring of the flat (N+1)^2 array u -> (4, N+1), the corner entries of
    the column sides holding the corner values (what mgx_get_boundary
    returns)."""
    U = u.reshape(N + 1, N + 1)
    return np.ascontiguousarray(np.stack([U[0, :], U[N, :], U[:, 0], U[:, N]]))


TOL = 1e-9

# Every (N, L, params, field, tower, fp modes, sequence, source) that
# tests/test_gpu_boundary.py runs through mg_outer; tests/test_boundary_fields.py
# checks on the checker alone that no per-cycle norm of these sits within
# fields.MARGIN of TOL.  sequence: per step the index k of the ring set for it
# (ring(N, k)), or None for a step with nothing set.  source: the step adds the
# separable source of source_factors(N).  tower 0 / 1: reference / correct; fp
# 0 / 1: bitwise / fma.
RING3 = (0, 1, 2)
CASES = [
    (128, 3, "easy", "generic", 0, (0, 1), RING3, False),
    (128, 3, "easy", "generic0", 0, (0, 1), RING3, False),
    (128, 3, "easy", "generic", 0, (0, 1), RING3, True),
    (256, 4, "easy", "generic", 0, (1,), RING3, False),
    (1024, 6, "easy", "generic", 0, (0, 1), RING3, False),
    (1024, 6, "easy", "generic0", 0, (0, 1), RING3, False),
    (1024, 6, "easy", "generic", 1, (1,), RING3, False),
    (4096, 6, "easy", "generic", 0, (1,), RING3, False),
    (4096, 7, "easy", "generic", 0, (0, 1), RING3, False),
    (4096, 7, "stiff", "generic", 0, (0, 1), RING3, False),
    (8192, 8, "easy", "generic", 0, (1,), (None, None, 0, None), False),
]


def source_factors(N):
    """-> (a, b): the one-term separable source f = a x b of the source case, a
    bump emitter of O(10) (dt f is O(1e-2) of u at the easy time step)."""
    x = np.arange(N + 1) / N
    a = 8.0 * np.exp(-40 * (x - .35) ** 2)
    b = 1.0 + .5 * np.cos(5 * x)
    return a, b


def checker_steps(run, seq, tol=TOL, source=None, keep_u=True):
    """The meaning of a step with a ring pending, on a fields.CheckerRun: rhs()
    with the old ring (+ fl(fl(dt) * f) on the interior for a source f, flat
    (N+1)^2), the new ring, then mg_outer with its own initial norm.
    -> [(cycles, r0, norms, u after the step or None)] per step of seq."""
    N = run.N
    out = []
    for k in seq:
        run.rhs()
        if source is not None:
            R = run.t.rhsfine.reshape(N + 1, N + 1)
            R[1:N, 1:N] += (np.float64(run.dt) * source.reshape(N + 1, N + 1))[1:N, 1:N]
        if k is not None:
            put(run.u, N, ring(N, k))
        cyc, r0, norms = run.mg_outer(tol)
        out.append((cyc, r0, norms, run.u.copy() if keep_u else None))
    return out


def corner_rule(g, N):
    """g as get(put(u, N, g), N) returns it: entries 0 and N of the column
    sides replaced by the rows' corner values."""
    g = np.array(g, dtype=np.float64).reshape(4, N + 1)
    g[2, 0], g[2, N] = g[0, 0], g[1, 0]
    g[3, 0], g[3, N] = g[0, N], g[1, N]
    return g

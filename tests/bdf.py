"""The meaning of variable-step BDF2 steps on a history (mgx_step_bdf2) on the
CPU checker (numpy only; run on a fields.CheckerRun, built on tsteps).

A sequence mixes theta-steps ("t", m, theta) -- tsteps' (m, theta) -- and BDF2
steps ("b", m); dt = m * dt0 with dt0 = fields.params(pname, N)[0].  A BDF2
step with the step before it of size dt_prev is, all np.float64 and every
operation rounded (the order include/mgx.h states),

    w  = dt / dt_prev        p = 1 + w        q = 1 + 2 w
    g  = p / q               b0 = (p p) / q   b1 = (w w) / q
    kA = (2 g) dt            c  = (g dt) s

    rhs = fl(fl(b0 u^n) - fl(b1 u^(n-1)))  (+ fl(c f))   on the interior,

a pending ring, then mg_outer with k = kA.  The first step of every sequence
makes no call at all on the solver, so it must be ("t", 1, .5).
"""
import numpy as np

import rings as R
import tsteps as T

TOL = T.TOL


def t(m, theta):
    return ("t", m, theta)


def b(m):
    return ("b", m)


SEQ = (t(1, .5), b(1), b(1), b(2), b(.5), t(.5, 1), b(1), b(1.5))
SEQ_R1 = (t(1, .5), b(1), b(1), b(1.5), b(.5), t(.5, 1), b(1), b(1.5))
SEQ_STIFF = (t(1, .5), b(1), b(.5), b(1), t(.5, 1), b(.7))   # N=4096 only

# the rings of the source case: per step of SEQ the index k of rings.ring(N, k)
# set "next", or None -- two BDF2 steps and the theta-step in the middle
RINGS = (None, 0, None, 1, None, 2, None, None)

# Every (N, L, params, field, tower, fp modes, sequence, extra[, nsmooth, fuse,
# shape]) that tests/test_gpu_bdf.py runs against the checker; tests/test_bdf_fields.py holds
# the margins on the checker alone.  tower 0 / 1: reference / correct; fp 0 / 1:
# bitwise / fma; extra: the separable source of rings.source_factors, scale 1,
# plus the rings RINGS.
CASES = [
    (128, 3, "easy", "generic", 0, (0, 1), SEQ, False),
    (128, 3, "easy", "generic0", 0, (0,), SEQ, False),
    (128, 3, "easy", "generic", 0, (0,), SEQ, True),
    (256, 4, "easy", "generic", 0, (1,), SEQ, False),
    (1024, 6, "easy", "generic", 0, (0, 1), SEQ, False),
    (1024, 6, "easy", "generic", 1, (1,), SEQ, False),
    (4096, 7, "easy", "generic", 0, (0, 1), SEQ, False),
    (4096, 7, "easy", "rank1", 0, (1,), SEQ_R1, False),
    (4096, 7, "stiff", "generic", 0, (1,), SEQ_STIFF, False),
    # other schedules (nsmooth, fuse, shape after the eight fields above; the
    # defaults are 3, 3, 1): a W-cycle context whose coarsest level (n = 32) is
    # solved inside the pair pass of the level above it -- theta-steps, BDF2
    # steps, pending rings and a source in one run -- and a context whose
    # smoothings are two passes of one sweep
    (256, 4, "easy", "generic", 0, (0, 1), SEQ, True, 3, 3, 2),
    (128, 3, "easy", "generic", 0, (0, 1), SEQ, False, 2, 1, 1),
]
SCHEDULE = (3, 3, 1)   # nsmooth, fuse, shape of a case that names none


def _expand(cases):
    out = []
    for c in cases:
        N, L, p, f, tw, fps, seq, ex = c[:8]
        for fp in fps:
            out.append((N, L, p, f, tw, fp, seq, ex) + (tuple(c[8:]) or SCHEDULE))
    return out


def _id(N, L, p, f, tw, fp, seq, ex, nsmooth, fuse, shape):
    sched = "" if (nsmooth, fuse, shape) == SCHEDULE else "-s%df%d-%s" % (
        nsmooth, fuse, "W" if shape == 2 else "V")
    return "N%d-L%d-%s-%s-t%d-%s%s%s" % (N, L, p, f, tw, "bitwise" if fp == 0 else "fma",
                                         "-source-rings" if ex else "", sched)


# (N, L, params, field, tower, fp, sequence, extra, nsmooth, fuse, shape)
CASE_PARAMS = _expand(CASES)
CASE_IDS = [_id(*c) for c in CASE_PARAMS]
CASE_ARGS = "N,L,pname,name,tower,fp,seq,extra,nsmooth,fuse,shape"


def coefs(dt, dt_prev):
    """-> (g, b0, b1, kA) as np.float64, every operation rounded."""
    dt, dt_prev = np.float64(dt), np.float64(dt_prev)
    one, two = np.float64(1.0), np.float64(2.0)
    w = dt / dt_prev
    p = one + w
    q = one + two * w
    g = p / q
    b0 = (p * p) / q
    b1 = (w * w) / q
    kA = (two * g) * dt
    return g, b0, b1, kA


def step_dt(dt0, m):
    return np.float64(m) * np.float64(dt0)


def bdf_rhs(rhs, u, h, N, b0, b1, f=None, c=None):
    """The BDF2 right-hand side into the interior of the flat array rhs (in
    place; its boundary entries stay): fl(fl(b0 u) - fl(b1 h)) (+ fl(c f))."""
    w = N + 1
    U, H = u.reshape(w, w), h.reshape(w, w)
    r = np.float64(b0) * U - np.float64(b1) * H
    if f is not None:
        r = r + np.float64(c) * f.reshape(w, w)
    rhs.reshape(w, w)[1:N, 1:N] = r[1:N, 1:N]
    return rhs


def checker_steps(run, dt0, seq, tol=TOL, source=None, rings=None, scale=1.0, keep_u=True):
    """seq on a fields.CheckerRun.  The checker keeps u^n and dt_prev itself:
    every step begins with h = u; a theta-step then is tsteps.checker_steps'
    (compute_rhs with k = kB, + fl(dt * f), the ring, mg_outer with k = kA); a
    BDF2 step writes bdf_rhs into run.t.rhsfine, the ring rings[i] if one is
    pending, and calls mg_outer with run.dt = kA.
    -> [(cycles, r0, norms, u after the step or None)]."""
    N = run.N
    out = []
    h_prev, dt_prev = None, None
    for i, st in enumerate(seq):
        dt = step_dt(dt0, st[1])
        un = run.u.copy()
        if st[0] == "t":
            kA, kB = T.k_pair(dt, st[2])
            run.dt = float(kB)
            run.rhs()
            if source is not None:
                Rr = run.t.rhsfine.reshape(N + 1, N + 1)
                Rr[1:N, 1:N] += ((np.float64(dt) * np.float64(scale))
                                 * source.reshape(N + 1, N + 1))[1:N, 1:N]
        else:
            assert h_prev is not None, "a BDF2 step needs a step before it"
            g, b0, b1, kA = coefs(dt, dt_prev)
            c = (g * dt) * np.float64(scale)
            bdf_rhs(run.t.rhsfine, un, h_prev, N, b0, b1, source, c)
        if rings is not None and rings[i] is not None:
            R.put(run.u, N, R.ring(N, rings[i]))
        run.dt = float(kA)
        cyc, r0, norms = run.mg_outer(tol)
        out.append((cyc, r0, norms, run.u.copy() if keep_u else None))
        h_prev, dt_prev = un, dt
    return out


def solver_steps(mg, dt0, seq, tol=TOL, rings=None, N=None, keep_u=True):
    """seq on a Multigrid with a history on: set_time_step before every step but
    the first (which must be ("t", 1, .5)), a pending ring where rings says so,
    step_ex or step_bdf2 -> [(cycles, res0, res, u or None)]."""
    out = []
    for i, st in enumerate(seq):
        dt = float(step_dt(dt0, st[1]))
        if i == 0:
            assert st == ("t", 1, .5)
        elif st[0] == "t":
            mg.set_time_step(dt, st[2])
        else:
            mg.set_time_step(dt)
        if rings is not None and rings[i] is not None:
            mg.set_boundary(R.ring(N, rings[i]), "next")
        cyc, r0, r = mg.step_ex(tol) if st[0] == "t" else mg.step_bdf2(tol)
        out.append((cyc, r0, r, mg.download() if keep_u else None))
    return out

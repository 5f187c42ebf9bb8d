"""The meaning of a theta-scheme step (mgx_set_time_step) on the CPU checker
(numpy only; built on fields.CheckerRun).

A step is given as (m, theta): dt = m * dt0 with dt0 = fields.params(pname,
N)[0], and

    kA = fl(fl(2 * theta) * dt)          the solve side: mg_outer with k = kA
    kB = fl(fl(2 * fl(1 - theta)) * dt)  the right-hand side: compute_rhs with k = kB

in np.float64, the order include/mgx.h states.  theta = .5 gives kA == kB ==
dt exactly (2 * .5 and 2 * (1 - .5) are exactly 1).  The first step of every
sequence makes no call at all on the solver, so it must be (1, .5).
"""
import numpy as np

import fields as F
import rings as R

TOL = 1e-9

SEQ_EASY = ((1, .5), (1, 1), (.5, 1), (2, .5), (3, .75), (1, .5))
SEQ_STIFF = ((1, .5), (.5, 1), (.25, 1), (.7, .6), (1, .5))   # N=4096 only
# the step-fusion comparison at N=8192, L=8 (solver against solver; on the
# checker: 2, 3, 3, 4, 2 cycles, margin 0.13)
SEQ_FUSE = ((1, .5), (2, .5), (2, .5), (1, 1), (1, .5))

# the rings of the source + ring case: per step the index k of rings.ring(N, k)
# set "next", or None
RINGS = (None, 0, None, 1, 2, None)

# Every (N, L, params, field, tower, fp modes, sequence, extra[, nsmooth, fuse,
# shape]) that tests/test_gpu_time_step.py runs against the checker; tests/
# test_time_step_fields.py holds the margins on the checker alone.  tower 0 / 1:
# reference / correct; fp 0 / 1: bitwise / fma; extra: the separable source of
# rings.source_factors plus the rings RINGS.
CASES = [
    (128, 3, "easy", "generic", 0, (0, 1), SEQ_EASY, False),
    (128, 3, "easy", "generic0", 0, (0, 1), SEQ_EASY, False),
    (128, 3, "easy", "generic", 0, (0, 1), SEQ_EASY, True),
    (256, 4, "easy", "generic", 0, (1,), SEQ_EASY, False),
    (1024, 6, "easy", "generic", 0, (0, 1), SEQ_EASY, False),
    (1024, 6, "easy", "generic", 1, (1,), SEQ_EASY, False),
    (4096, 6, "easy", "generic", 0, (1,), SEQ_EASY, False),
    (4096, 7, "easy", "generic", 0, (0, 1), SEQ_EASY, False),
    (4096, 7, "easy", "rank1", 0, (1,), SEQ_EASY, False),
    (4096, 7, "stiff", "generic", 0, (0, 1), SEQ_STIFF, False),
    # other schedules (nsmooth, fuse, shape after the eight fields above; the
    # defaults are 3, 3, 1): a W-cycle context whose coarsest level (n = 32) is
    # solved inside the pair pass of the level above it, with the source and
    # the rings, and a context whose smoothings are two passes of one sweep
    # (generic0: on generic the (3, .75) step, 17 cycles, has a norm within
    # 0.6 % of the tolerance)
    (256, 4, "easy", "generic", 0, (0, 1), SEQ_EASY, True, 3, 3, 2),
    (128, 3, "easy", "generic0", 0, (0, 1), SEQ_EASY, False, 2, 1, 1),
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


def k_pair(dt, theta):
    """-> (kA, kB) as np.float64, every product rounded."""
    dt, theta = np.float64(dt), np.float64(theta)
    kA = (np.float64(2.0) * theta) * dt
    kB = (np.float64(2.0) * (np.float64(1.0) - theta)) * dt
    return kA, kB


def source_field(N):
    """-> (a, b, f): rings.source_factors and f = fl(a_i * b_j), flat."""
    a, b = R.source_factors(N)
    return a, b, (a[:, None] * b[None, :]).ravel()


def checker_steps(run, dt0, seq, tol=TOL, source=None, rings=None, keep_u=True):
    """seq on a fields.CheckerRun: per step (m, theta), dt = m * dt0,
      1. compute_rhs with k = kB,
      2. + fl(dt * f) on the interior for a source f (flat (N+1)^2),
      3. the ring rings[i] (rings.ring(N, k)), if one is pending,
      4. mg_outer with k = kA (its initial norm in the reference's term order).
    -> [(cycles, r0, norms, u after the step or None)]; run.dt is left at the
    last kA."""
    N = run.N
    out = []
    for i, (m, theta) in enumerate(seq):
        dt = np.float64(m) * np.float64(dt0)
        kA, kB = k_pair(dt, theta)
        run.dt = float(kB)
        run.rhs()
        if source is not None:
            Rr = run.t.rhsfine.reshape(N + 1, N + 1)
            Rr[1:N, 1:N] += (np.float64(dt) * source.reshape(N + 1, N + 1))[1:N, 1:N]
        if rings is not None and rings[i] is not None:
            R.put(run.u, N, R.ring(N, rings[i]))
        run.dt = float(kA)
        cyc, r0, norms = run.mg_outer(tol)
        out.append((cyc, r0, norms, run.u.copy() if keep_u else None))
    return out


def solver_steps(mg, dt0, seq, tol=TOL, rings=None, N=None, keep_u=True, first_call=False):
    """seq on a Multigrid: set_time_step before every step but the first (which
    must be (1, .5) unless first_call), a pending ring where rings says so,
    step_ex -> [(cycles, res0, res, u or None)]."""
    out = []
    for i, (m, theta) in enumerate(seq):
        if i > 0 or first_call:
            mg.set_time_step(float(np.float64(m) * np.float64(dt0)), theta)
        else:
            assert (m, theta) == (1, .5)
        if rings is not None and rings[i] is not None:
            mg.set_boundary(R.ring(N, rings[i]), "next")
        cyc, r0, r = mg.step_ex(tol)
        out.append((cyc, r0, r, mg.download() if keep_u else None))
    return out

"""The meaning of a predicted start for BDF2 steps (mgx_set_predictor,
include/mgx.h) on the CPU checker (numpy only; fields.CheckerRun, built on bdf
and dense).

A sequence is bdf's -- ("t", m, theta) and ("b", m) -- and a BDF2 step may
carry a third entry True, "reverse the velocity before it": mgx_set_velocity(
-v1, -v2) on the solver, a fresh CheckerRun with the negated fields and the
current u on the checker.  The extrapolation then points the wrong way, which
is the small-size way to a refused guess.

A BDF2 step with the predictor at order q > 0 and no ring pending:
    e   = 2 if q == 2, the history is two deep and holds u^(n-2), else 1
    g   = dense.reference(u^n, u^(n-1), u^(n-2), e, +dt, dt_prev, dt_prev2) on
          rows and columns 1..N-1, u^n on the ring
    rhs = bdf.bdf_rhs, k = kA
    r0  = |rhs - A u^n|, rp = |rhs - A g|     (both in the reference's term order)
    adopted = rp < r0;  u = g and res = rp if adopted, else u = u^n and res = r0
    while cycles < 50 and res / r0 > tol: a cycle
A step that takes a pending ring, and every step at order 0, is bdf's.
"""
from collections import namedtuple

import numpy as np

import bdf as B
import dense as D
import fields as F
import rings as R
import tsteps as T

TOL = B.TOL
MAX_CYCLE = 50

# cyc, r0, norms: as bdf.checker_steps (norms = the norm after every cycle; the
# checker's are fields.Norm); res: the last norm (rp or r0 where no cycle ran);
# u: after the step; e: the effective order (0: unpredicted); adopted; rp (None
# where e == 0); un, h: u^n and u^(n-1) as the history holds them after the
# step (h None where the history is one deep or u^(n-1) is not valid)
Step = namedtuple("Step", "cyc r0 norms res u e adopted rp un h")


def rb(m):
    """A BDF2 step with the velocity reversed before it."""
    return ("b", m, True)


def reversed_at(seq, k):
    return tuple(rb(s[1]) if i == k else s for i, s in enumerate(seq))


def smooth_u0(N):
    """sin(pi x) sin(2 pi y) + 0.3: smooth, with a non-zero ring."""
    x = np.arange(N + 1) / N
    u = np.sin(np.pi * x)[:, None] * np.sin(2 * np.pi * x)[None, :] + .3
    return np.ascontiguousarray(u).ravel()


def make(name, N):
    """fields.make plus "smooth": smooth_u0 with generic's velocity."""
    if name == "smooth":
        _, v1, v2 = F.make("generic", N)
        return smooth_u0(N), v1, v2
    return F.make(name, N)


def guess(un, h, h2, N, e, dt, dt1, dt2):
    """g: the interpolant one step ahead on the interior, u^n's bits on the ring."""
    w = N + 1
    full = D.reference(un, h, h2, e, float(dt), float(dt1), float(dt2) if e == 2 else 0.0)
    g = np.array(un, dtype=np.float64).reshape(w, w).copy()
    g[1:N, 1:N] = full.reshape(w, w)[1:N, 1:N]
    return g.ravel()


def ratios(st, tol=TOL):
    """Every r / r0 of a step that decides something: the start's and each cycle's."""
    out = [float(n) / float(st.r0) for n in st.norms]
    if st.e:
        out.append(float(st.rp) / float(st.r0))
    return out


def margin(st, tol=TOL):
    """The smallest distance of a deciding ratio from tol (relative to tol), and
    on a predicted step of rp / r0 from 1."""
    m = min([abs(r / tol - 1.0) for r in ratios(st, tol)] or [1.0])
    if st.e:
        m = min(m, abs(float(st.rp) / float(st.r0) - 1.0))
    return m


def checker_steps(O, u0, v1, v2, N, L, dt0, nu, seq, order, depth=2, tol=TOL, tower=0, fp=0,
                  source=None, rings=None, scale=1.0, sched=B.SCHEDULE, linear_at=()):
    """seq on the checker with the predictor at `order` and a history `depth`
    deep -> [Step].  The caller has set the checker's fp mode and threads.
    linear_at: the steps before which u^(n-2) is not valid, as after the
    mgx_rollback of a step that is not part of seq."""
    def new_run(u, sign):
        return F.CheckerRun(O, u, sign * np.asarray(v1), sign * np.asarray(v2), N, L, float(dt0),
                            nu, tower, sched[0], sched[2], fp)
    sign = 1.0
    run = new_run(np.array(u0), sign)
    out = []
    h, dt1, h2, dt2 = None, None, None, None   # u^(n-1), its step; u^(n-2), its step
    try:
        for i, st in enumerate(seq):
            dt = B.step_dt(dt0, st[1])
            if len(st) > 2 and st[0] == "b" and st[2]:
                sign = -sign
                u = run.u.copy()
                run.close()
                run = new_run(u, sign)
            un = run.u.copy()
            ring = rings is not None and rings[i] is not None
            e, adopted, rp = 0, False, None
            if i in linear_at:
                h2, dt2 = None, None
            if st[0] == "t":
                kA, kB = T.k_pair(dt, st[2])
                run.dt = float(kB)
                run.rhs()
                if source is not None:
                    Rr = run.t.rhsfine.reshape(N + 1, N + 1)
                    Rr[1:N, 1:N] += ((np.float64(dt) * np.float64(scale))
                                     * source.reshape(N + 1, N + 1))[1:N, 1:N]
            else:
                assert h is not None, "a BDF2 step needs a step before it"
                g_, b0, b1, kA = B.coefs(dt, dt1)
                c = (g_ * dt) * np.float64(scale)
                B.bdf_rhs(run.t.rhsfine, un, h, N, b0, b1, source, c)
                if order > 0 and not ring:
                    e = 2 if order == 2 and depth == 2 and h2 is not None else 1
            if ring:
                R.put(run.u, N, R.ring(N, rings[i]))
            run.dt = float(kA)
            if e:
                r0 = run.norm(reference_form=True)
                run.u[:] = guess(un, h, h2, N, e, dt, dt1, dt2)
                rp = run.norm(reference_form=True)
                adopted = bool(rp < r0)
                if not adopted:
                    run.u[:] = un
                res, norms = (rp if adopted else r0), []
                while len(norms) < MAX_CYCLE and res / r0 > tol:
                    res = run.cycle()
                    norms.append(res)
                cyc = len(norms)
            else:
                cyc, r0, norms = run.mg_outer(tol, MAX_CYCLE)
                res = norms[-1] if norms else r0
            if depth == 2:
                h2, dt2 = h, dt1
            h, dt1 = un, dt
            out.append(Step(cyc, r0, norms, res, run.u.copy(), e, adopted, rp, un, h2))
    finally:
        run.close()
    return out


def solver_steps(mg, dt0, seq, v1, v2, tol=TOL, rings=None, N=None, probe=None, first=True):
    """seq on a Multigrid whose history and predictor the caller has set:
    bdf.solver_steps plus the reversals -> [Step] (norms = None; un, h = fields
    5 and 6 of sample(1) after the step, h None where history2 is not valid);
    probe(mg, i): called after step i, its result appended to a second list;
    first=False: seq continues a run, so its first step sets its dt too."""
    out, probed = [], []
    sign = 1.0
    for i, st in enumerate(seq):
        dt = float(B.step_dt(dt0, st[1]))
        if i == 0 and first:
            assert st == ("t", 1, .5)
        elif st[0] == "t":
            mg.set_time_step(dt, st[2])
        else:
            mg.set_time_step(dt)
        if len(st) > 2 and st[0] == "b" and st[2]:
            sign = -sign
            mg.set_velocity(sign * np.asarray(v1), sign * np.asarray(v2))
        if rings is not None and rings[i] is not None:
            mg.set_boundary(R.ring(N, rings[i]), "next")
        cyc, r0, r = mg.step_ex(tol) if st[0] == "t" else mg.step_bdf2(tol)
        info = mg.predictor_info()
        if st[0] == "t":
            info = dict(info, last_order=0, adopted=0, res_pred=0.0)   # (the last BDF2 step's)
        un = mg.sample(1, "history").ravel()
        hd = mg.history_depth()
        h = mg.sample(1, "history2").ravel() if hd["depth"] == 2 and hd["valid2"] else None
        out.append(Step(cyc, r0, None, r, mg.download(), info["last_order"], bool(info["adopted"]),
                        info["res_pred"] if info["last_order"] else None, un, h))
        if probe is not None:
            probed.append(probe(mg, i))
    return (out, probed) if probe is not None else out


# ---- the cases tests/test_gpu_predict.py runs against the checker;
# tests/test_predict_fields.py holds their margins on the checker alone.
# (N, L, params, field, fp, sequence, order, extra); extra: None, "sep-rings" (the
# separable source of rings.source_factors plus the rings bdf.RINGS) or "field"
# (the same source as an array).  The history is two deep at order 2 and one
# deep at order 1.
SEQ_REV = reversed_at(B.SEQ, 3)
CASES = [
    (8, 2, "easy", "generic", 0, B.SEQ, 1, None),
    (8, 2, "easy", "generic", 0, B.SEQ, 2, None),
    (128, 3, "easy", "smooth", 0, B.SEQ, 1, None),
    (128, 3, "easy", "smooth", 0, B.SEQ, 2, None),
    (32, 2, "easy", "generic", 0, B.SEQ, 2, None),
    (32, 2, "easy", "generic", 0, SEQ_REV, 2, None),
    (128, 3, "easy", "generic", 0, B.SEQ, 2, None),
    (128, 3, "easy", "generic", 1, B.SEQ, 2, None),
    (128, 3, "easy", "generic", 0, SEQ_REV, 2, None),
    (128, 3, "easy", "generic", 1, SEQ_REV, 2, None),
    (128, 3, "easy", "generic", 0, B.SEQ, 2, "sep-rings"),
    (128, 3, "easy", "generic", 1, B.SEQ, 1, "field"),
    (1024, 6, "easy", "generic", 1, B.SEQ, 1, None),
    (4096, 7, "easy", "rank1", 1, B.SEQ_R1, 2, None),
    (4096, 7, "stiff", "generic", 1, B.SEQ_STIFF, 2, None),
]
# the cases whose total cycle count must be strictly below the plain run's, as
# (N, L, params, field, fp, sequence, extra) -- at both orders
GAINS = [(8, 2, "easy", "generic", 0, B.SEQ, None), (128, 3, "easy", "smooth", 0, B.SEQ, None)]
CASE_ARGS = "N,L,pname,name,fp,seq,order,extra"


def case_id(N, L, pname, name, fp, seq, order, extra):
    return "N%d-L%d-%s-%s-%s-q%d%s%s" % (N, L, pname, name, "bitwise" if fp == 0 else "fma", order,
                                         "-rev" if any(len(s) > 2 and s[2] is True and s[0] == "b"
                                                       for s in seq) else "",
                                         "-" + extra if extra else "")


CASE_IDS = [case_id(*c) for c in CASES]

# Reject and retry (easy, generic, order 2): RETRY_PREFIX, a BDF2 step of twice
# the size that is rolled back and is no part of the checker's run, then
# retry_tail(depth) -- at depth 2 a BDF2 step of half the size that predicts
# linearly (u^(n-2) went with the rollback: linear_at), at depth 1, where the
# rollback leaves no valid history, an implicit Euler step.  (N, L, fp, depth)
RETRY_PREFIX = (B.t(1, .5), B.b(1), B.b(1))
RETRY_CASES = [(128, 3, 0, 1), (128, 3, 0, 2), (1024, 6, 1, 1), (1024, 6, 1, 2)]


def retry_tail(depth):
    return (B.b(.5), B.b(1), B.b(1)) if depth == 2 else (B.t(.5, 1.0), B.b(1), B.b(1))


def case_extra(extra, N):
    """-> (source array or None, rings or None, solver setter)."""
    if extra is None:
        return None, None, lambda mg: None
    a, b, f = T.source_field(N)
    if extra == "sep-rings":
        return f, B.RINGS, lambda mg: mg.set_source_separable(a, b)
    assert extra == "field"
    return f, None, lambda mg: mg.set_source(f)


def run_case(O, N, L, pname, name, fp, seq, order, extra, tol=TOL):
    """checker_steps of one case (the caller has set threads and fp mode)."""
    dt, nu = F.params(pname, N)
    u0, v1, v2 = make(name, N)
    src, rings, _ = case_extra(extra, N)
    return checker_steps(O, u0, v1, v2, N, L, dt, nu, seq, order, 2 if order == 2 else 1, tol,
                         fp=fp, source=src, rings=rings)

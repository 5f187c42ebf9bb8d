"""The solver's exits -- the cycle cap, the limits of the coarsest solve, a
non-finite field -- as cases and checker sequences that the CPU file
(tests/test_exits_fields.py) and the GPU file (tests/test_gpu_exits.py) share
(numpy only, in the style of tests/schedules.py and tests/fields.py).

or_mg_inner (oracle/mg_oracle.c) hard-codes the coarsest solve's limits, 1000
sweeps and 1e-5, so mg_inner() below mirrors it (multigrid.cpp:52-90) line for
line from the checker's own operators, with the two limits as parameters, and
records the norm of every coarsest iteration and the iteration count of every
coarsest visit.  tests/test_exits_fields.py pins it bit for bit to
oracle.Tower.mg_inner at the defaults.  Run is a fields.CheckerRun whose cycles
are that mirror.

A count is only comparable where the decision it rests on does not hinge on a
summation order: as fields.MARGIN (1 %) holds for every r_k / r_0 of a cycle
count, it must hold for every coarsest norm against coarse_tol before a
coarsest iteration count is compared (coarse_margin).  The CPU file asserts
both for every case here.

Cycle-cap cases (CAP_*).  Checker figures (seed 1), r_k / r_0:
  N=4096 L=5 generic stiff, reference tower, fma (CAP_MAIN): r_0 = 1535, c* = 6:
    3.79e-3 1.33e-4 5.75e-6 2.69e-7 1.31e-8 6.50e-10 (margin 0.35; bitwise mode the
    same to three digits).  The second mg_outer starts from r_m and ends capped
    for every m -- after m = 5 it would need 1.3e-17 r_0, below the rounding
    floor of 5e-16 r_0 -- its r_k / r_m: m = 1: 3.5e-2; m = 2: 4.3e-2 2.0e-3;
    m = 5: 5.0e-2 2.5e-3 1.3e-4 6.7e-6 3.5e-7; m = 6 and 7 (from r_6): 5.1e-2
    2.6e-3 1.3e-4 7.0e-6 5.2e-7 8.7e-8 1.1e-8 (bitwise mode: ... 7.0e-6 9.0e-7
    8.0e-7: the floor); the nearest any comes to 1e-9 is a factor 10.7.
  correct tower: c* = 6, 3.33e-3 1.09e-4 4.50e-6 2.03e-7 9.58e-9 4.64e-10 (0.54)
  W-cycles, L=4 (CAP_W): c* = 3, 1.33e-4 2.68e-7 6.49e-10 (0.35); from r_3: 2.6e-3
    7.0e-6 8.7e-8 3.4e-9 (a factor 3.4 from 1e-9)
  N=512 L=5 visc16 fma, tol 1e-6 (CAP_SMALL): r_0 = 187, 4.21e-3 1.58e-4, then from
    r_2: 4.5e-2 2.1e-3
  N=512 L=5 stiff (CAP_GROWTH): r_0 = 47.1, 8.4 5.2e2 4.5e4 4.4e6, then from r_4 =
    2.1e8: 1.0e2 1.2e4 1.3e6 1.5e8
  N=4096 L=5 grow3 fma (CAP_GROWTH_CROSS): r_0 = 22523, 1.38e-2 7.89e-3 8.39e-3
    1.09e-2 (falls, then grows), then from r_4 = 246: 1.41 2.06 3.07 4.65 -- the
    extrapolation r_k (r_k / r_(k-1)) of op_mg_outer sees factors above 1
  three stiff steps at N=4096 under max_cycle 2 (CAP_STEPS): r_0 = 1535, 981, 647;
    r_2 / r_0 = 1.33e-4 1.54e-4 1.73e-4 (uncapped: 6 cycles each)
  N=8192 L=6 easy bitwise (CAP_STEPS_SLOW): 2 cycles per step, 8.6e-6 2.2e-10 and
    7.2e-6 1.8e-10 (0.78, 0.82; tests/test_gpu_generic_fields.py)
  N=128 L=3 visc16 bitwise, tol 1e-9 (CAP_TIMESTEPPER): c* = 7 in each of three
    steps (last 1.2e-10 1.8e-10 2.6e-10, margin 0.74); under max_cycle 2: r_2 / r_0
    = 4.0e-4 6.3e-4 9.0e-4
Coarsest-solve limits (COARSE_FORMS x limits()).  The sequence is rhs and two
run_cycles(1).  Per form the checker's coarsest norms of the first visit with
the default limits, from which the loose and the tight coarse_tol are taken,
and the iteration counts per visit (both cycles) with each:
  (coarse_params: 0.57 a sweep on every form; identical in both fp modes to the
  digits shown; margin = coarse_margin, the smallest over all visits)
  n=64 of N=256 L=3 (lds_fused, lds, l2_n64): 3.34 1.80 1.00 0.566 0.320 0.182 ...
    1.34e-5 7.68e-6: 24 sweeps, 25 in cycle 2; loose 0.5: 5, 5 (margin 0.098);
    tight 1e-6: 28, 29 (0.171)
  n=256 of N=512 L=2 (l2_n256): 7.18 2.89 1.42 0.754 ... 1.08e-5 6.24e-6: 25, 23;
    loose 0.25: 6, 5 (0.079); tight 1e-6: 29, 27 (0.091)
  n=512 of N=1024 L=2 (host_loop): 13.5 4.99 2.30 1.15 ... 1.26e-5 7.24e-6: 25, 23;
    loose 0.5: 6, 4 (0.164); tight 2e-6: 28, 26 (0.093)
  n=64, L=1 (finest): 6.50 2.84 1.52 0.843 ... 1.62e-5 9.06e-6: 24, then 1 (the
    second cycle starts converged); loose 0.5: 5, 1 (0.051); tight 1e-6: 28, 1 (0.109)
  W-cycle, n=64 of N=256 L=3 (w_cycle, w_cycle_fused), 8 visits a cycle: 24 1 23 1
    23 1 21 1 | 22 1 20 1 20 1 19 1; loose 0.3: 6 1 4 1 5 1 3 1 | 4 1 2 1 3 1 1 1
    (0.057); tight 1.2e-6: 28 1 26 1 27 1 25 1 | 25 1 24 1 24 1 23 1 (0.056).  The
    second visit of a pair starts from the first one's solution: one sweep.
    Under a sweep cap every visit runs the cap: 7 7 7 7 ...
  n=64 of N=1024 L=5, two parts (replicated): 7.21 4.03 2.28 ... 9.91e-6: 25, 29 (the
    cycles do not contract at this stiffness: finest norms 1295, 1682); loose 0.5:
    6, 10 (0.167); tight 2e-6: 28, 32 (0.070)
  n=64 of N=2048 L=6, four cycles (graph): 13.7 7.72 4.38 ... 6.22e-6: 27, 32, ..;
    finest norms 1.0e4 1.4e4 2.1e5 3.8e6; loose 0.4: 8, 13, 18, 23 (0.143); tight
    5e-5: 24, 29, 34, 39 (0.086; 1e-6 would take 46 sweeps in cycle 4)
  With coarse_maxit 1, 2, 7 and the default tolerance, and with 5 and tolerance 0,
  every visit of every form runs exactly the cap (norms above 2.8e-3 throughout).
"""
import collections
import ctypes as C

import numpy as np

import fields as F

REF, COR = 0, 1
BIT, FMA = 0, 1
V, W = 1, 2

COARSE_TOL, COARSE_MAXIT = 1e-5, 1000   # multigrid.cpp:58


# ---------------------------------------------------------------- the mirror

def _level(t, which, lvl):
    """Level lvl's array of a tower as a view of the checker's own memory (the
    first (n_l + 1)^2 entries: what mg_inner reads and writes there)."""
    if lvl == 0:
        return t._keep[{"u": 0, "v1": 1, "v2": 2, "rhs": 3}[which]]
    n = t.n >> lvl
    return np.ctypeslib.as_array(getattr(t, which)[lvl], shape=((n + 1) ** 2,))


def mg_inner(O, t, dt, nu, nsmooth=3, shape=1, coarse_tol=COARSE_TOL, coarse_maxit=COARSE_MAXIT,
             visits=None, norms=None, lvl=0, n=None, dx=None):
    """multigrid.cpp:52-90 on an oracle.Tower -> the sweeps of every coarsest
    solve (or_mg_inner's return value).  visits: a list that receives the
    iteration count of every coarsest visit; norms: one that receives, per
    visit, the list of the norms after each iteration."""
    lib, p = O.lib(), O._p
    n = t.n if n is None else n
    dx = 1.0 / t.n if dx is None else dx
    ui, rhsi, v1i, v2i = (_level(t, w, lvl) for w in ("u", "rhs", "v1", "v2"))
    cnt = (n + 1) * (n + 1)
    tmp = t.tmp[:cnt]            # (one scratch array for every level, as the reference's)
    nnew, dx2 = n // 2, 2 * dx
    coarse_iters = 0
    for _ in range(shape):
        if lvl == t.maxlvl - 1:
            res_exact, i, seen = 1.0, 0, []
            while i < coarse_maxit and res_exact > coarse_tol:
                O.gauss_seidel(ui, rhsi, n, v1i, v2i, dt, nu, dx)
                O.residual(ui, rhsi, n, v1i, v2i, dt, nu, dx, res=tmp)
                res_exact = O.compute_norm(tmp, n)
                seen.append(res_exact)
                i += 1
            coarse_iters += i
            if visits is not None:
                visits.append(i)
            if norms is not None:
                norms.append(seen)
        else:
            ui1, rhsi1 = _level(t, "u", lvl + 1), _level(t, "rhs", lvl + 1)
            for _it in range(nsmooth):
                O.gauss_seidel(ui, rhsi, n, v1i, v2i, dt, nu, dx)
            O.residual(ui, rhsi, n, v1i, v2i, dt, nu, dx, res=tmp)
            lib.or_restriction(p(rhsi1), p(tmp), C.c_long(n))
            ui1[:] = 0.0
            coarse_iters += mg_inner(O, t, dt, nu, nsmooth, shape, coarse_tol, coarse_maxit,
                                     visits, norms, lvl + 1, nnew, dx2)
            lib.or_prolongation(p(tmp), p(ui1), C.c_long(nnew))
            ui += tmp
            for _it in range(nsmooth):
                O.gauss_seidel(ui, rhsi, n, v1i, v2i, dt, nu, dx)
    return coarse_iters


class Run(F.CheckerRun):
    """A fields.CheckerRun whose cycles are the mirror, with the limits of the
    coarsest solve; .visits and .coarse_norms grow by one entry per coarsest
    visit."""

    def __init__(self, O, u0, v1, v2, N, L, dt, nu, tower=0, nsmooth=3, shape=1, fp=0,
                 coarse_tol=COARSE_TOL, coarse_maxit=COARSE_MAXIT):
        super().__init__(O, u0, v1, v2, N, L, dt, nu, tower, nsmooth, shape, fp)
        self.coarse_tol, self.coarse_maxit = coarse_tol, coarse_maxit
        self.visits, self.coarse_norms = [], []

    def mg_inner(self):
        self.coarse_its += mg_inner(self.O, self.t, self.dt, self.nu, self.nsmooth, self.shape,
                                    self.coarse_tol, self.coarse_maxit, self.visits,
                                    self.coarse_norms)

    def step(self, tol, max_cycle=50):
        self.rhs()
        return self.mg_outer(tol, max_cycle)


def coarse_margin(norms, tol):
    """The smallest |norm / tol - 1| over every iteration of every visit (inf
    for tol = 0: nothing is ever within reach of it)."""
    if tol == 0.0:
        return float("inf")
    return min(abs(r / tol - 1.0) for visit in norms for r in visit)


# ---------------------------------------------------------------- the cycle cap

CapCase = collections.namedtuple("CapCase", "N L params field tower fp shape form tol")
# (form: a name of schedules.FORMS, or None for the library's defaults)

TOL = F.TOL
CAP_MAIN = CapCase(4096, 5, "stiff", "generic", REF, FMA, V, None, TOL)
CAP_MAIN_CAPS = (1, 2, 5, 6, 7)       # c* = 6
CAP_KNOB_CAPS = (2, 6)
CAP_OTHER = [   # bitwise mode and the correct tower once each
    (CapCase(4096, 5, "stiff", "generic", REF, BIT, V, None, TOL), (2, 6)),
    (CapCase(4096, 5, "stiff", "generic", COR, FMA, V, None, TOL), (2, 6)),
]
CAP_W = CapCase(4096, 4, "stiff", "generic", REF, FMA, W, None, TOL)
CAP_W_CAPS = (1, 3, 4)                # c* = 3
# no cross pass below N = 4096: tiles and the forced march
CAP_SMALL = [(CapCase(512, 5, "visc16", "generic", REF, FMA, V, form, 1e-6), (2,))
             for form in ("tiles", "march")]
# "stiff" diverges below N = 2048 (tests/fields.py): the norms grow
CAP_GROWTH = CapCase(512, 5, "stiff", "generic", REF, FMA, V, None, TOL)
CAP_GROWTH_CAPS = (4,)
# with the cross pass and mg_outer's predicted stores: dt = 3 / N, nu = -2e-3
CAP_GROWTH_CROSS = CapCase(4096, 5, "grow3", "generic", REF, FMA, V, None, TOL)
CAP_STEPS = (CapCase(4096, 5, "stiff", "generic", REF, FMA, V, None, TOL), 3, 2)
CAP_STEPS_SLOW = CapCase(8192, 6, "easy", "generic", REF, BIT, V, None, TOL)   # c* = 2 per step
CAP_TIMESTEPPER = (CapCase(128, 3, "visc16", "generic", REF, BIT, V, None, 1e-9), 3, 2)


def cap_id(c):
    return "N%d-L%d-%s-%s-t%d-%s-%s%s" % (
        c.N, c.L, c.params, c.field, c.tower, "fma" if c.fp else "bitwise",
        "W" if c.shape == 2 else "V", "-" + c.form if c.form else "")


def cap_run(O, case, u0, v1, v2, **kw):
    dt, nu = F.params(case.params, case.N)
    return Run(O, u0, v1, v2, case.N, case.L, dt, nu, case.tower, 3, case.shape, case.fp, **kw)


def cap_sequence(run, caps, tol):
    """rhs; then per cap m of `caps`: mg_outer(tol) under max_cycle = m, and a
    second one continuing from its state -> dict: r0, norms (of the longest
    first mg_outer: min(max(caps), c*) cycles) and per m
      first = cycles of the first call, u1, second = (cycles, r0, norms), u2.
    The first calls are prefixes of one run (mg_outer leaves the right-hand
    side alone), the second ones start from the snapshots."""
    run.rhs()
    r0 = run.norm(reference_form=True)
    res, norms, snaps = r0, [], {}
    while len(norms) < max(caps) and res / r0 > tol:
        res = run.cycle()
        norms.append(res)
        if len(norms) in caps:
            snaps[len(norms)] = run.u.copy()
    snaps.setdefault(len(norms), run.u.copy())
    out = {"r0": r0, "norms": norms, "caps": {}}
    for m in caps:
        k = min(m, len(norms))
        run.u[:] = snaps[k]
        second = run.mg_outer(tol, m)
        out["caps"][m] = dict(first=k, u1=snaps[k], second=second, u2=run.u.copy())
    return out


def cap_steps_sequence(run, steps, max_cycle, tol):
    """`steps` time steps under the cap -> dict(outers = [(cycles, r0, norms)],
    u)."""
    outers = [run.step(tol, max_cycle) for _ in range(steps)]
    return dict(outers=outers, u=run.u.copy())


# ---------------------------------------------------------------- the coarsest solve

# name -> (N, L, shape, parts, fp modes, tuning keys); coarsest n = N >> (L - 1)
CoarseForm = collections.namedtuple("CoarseForm", "name N L shape parts fps keys cycles",
                                    defaults=(2,))
COARSE_FIELD = "generic"


def coarse_params(form):
    """-> (dt, nu): the stiff time step with a diffusion number dt |nu| / h^2 of
    1.6 on the COARSEST level (1.6 x 4^(L-1) on the finest).  With any set of
    fields.PARAMS the coarsest level of a tower is so far from stiff that its
    solve meets 1e-5 in one to four sweeps -- nothing for a sweep cap of 7 to
    end; with this one it takes 24 to 32 sweeps at 0.57 a sweep, on every
    form."""
    return 1.0 / form.N, -1.6 * 4 ** (form.L - 1) / form.N
COARSE_FORMS = [
    CoarseForm("lds_fused", 256, 3, V, 0, (BIT, FMA), dict(coarse_fuse=1, coarse_lds=1, tile_max_n=2048)),
    CoarseForm("lds", 256, 3, V, 0, (BIT, FMA), dict(coarse_fuse=0, coarse_lds=1)),
    CoarseForm("l2_n64", 256, 3, V, 0, (BIT, FMA), dict(coarse_fuse=0, coarse_lds=0)),
    CoarseForm("l2_n256", 512, 2, V, 0, (BIT, FMA), {}),
    CoarseForm("host_loop", 1024, 2, V, 0, (FMA,), {}),
    CoarseForm("finest", 64, 1, V, 0, (BIT,), {}),
    CoarseForm("w_cycle", 256, 3, W, 0, (FMA,), dict(coarse_fuse=0)),
    CoarseForm("w_cycle_fused", 256, 3, W, 0, (FMA,), dict(coarse_fuse=1, tile_max_n=2048)),
    CoarseForm("replicated", 1024, 5, V, 2, (FMA,), {}),
    CoarseForm("graph", 2048, 6, V, 0, (FMA,), dict(graph_level=1), 4),
]
# (graph: a sub-cycle is captured once per entry state -- the levels' current
# buffers and right-hand sides -- and those alternate from cycle to cycle, so
# cycles 1 and 2 are captures and 3 and 4 their replays: four cycles there.)
# (L = 1 runs the stand-alone residual kernels, which keep the reference's
# expressions in both fp modes -- tests/schedules.py -- so "finest" is a
# bitwise-mode case)

# per (N, L, shape): the loose and the tight coarse_tol (figures above)
COARSE_TOLS = {
    (256, 3, V): (0.5, 1e-6),
    (512, 2, V): (0.25, 1e-6),
    (1024, 2, V): (0.5, 2e-6),
    (64, 1, V): (0.5, 1e-6),
    (256, 3, W): (0.3, 1.2e-6),
    (1024, 5, V): (0.5, 2e-6),
    (2048, 6, V): (0.4, 5e-5),   # (four cycles whose norms grow: 1e-6 would take 46 sweeps)
}


def limits(form):
    """The (coarse_tol, coarse_maxit, how) of a form; how = "cap" (the sweep cap
    ends every visit) or "tol"."""
    loose, tight = COARSE_TOLS[form.N, form.L, form.shape]
    return [(COARSE_TOL, 1, "cap"), (COARSE_TOL, 2, "cap"), (COARSE_TOL, 7, "cap"),
            (loose, 50, "tol"), (tight, 50, "tol"), (0.0, 5, "cap")]


def coarse_run(O, form, fp, u0, v1, v2, coarse_tol, coarse_maxit):
    dt, nu = coarse_params(form)
    return Run(O, u0, v1, v2, form.N, form.L, dt, nu, REF, 3, form.shape, fp,
               coarse_tol=coarse_tol, coarse_maxit=coarse_maxit)


def coarse_sequence(run, cycles=2):
    """rhs; run_cycles(1) `cycles` times -> dict: norms, its (the running count after
    each call), visits (per cycle the iteration count of each visit),
    coarse_norms, u."""
    run.rhs()
    norms, its, visits = [], [], []
    for _ in range(cycles):
        seen = len(run.visits)
        norms.append(run.cycle())
        its.append(run.coarse_its)
        visits.append(run.visits[seen:])
    return dict(norms=norms, its=its, visits=visits, coarse_norms=list(run.coarse_norms),
                u=run.u.copy())


# ---------------------------------------------------------------- a NaN

NAN_N, NAN_L, NAN_PARAMS = 256, 3, "visc16"


def nan_field():
    """generic() with one NaN at the centre (an even row and column: the
    injection hands it to every level)."""
    u0, v1, v2 = F.make("generic", NAN_N)
    u0 = u0.copy()
    u0[(NAN_N // 2) * (NAN_N + 1) + NAN_N // 2] = np.nan
    return u0, v1, v2


def nan_run(O, u0, v1, v2):
    dt, nu = F.params(NAN_PARAMS, NAN_N)
    return Run(O, u0, v1, v2, NAN_N, NAN_L, dt, nu, REF, 3, V, BIT)


def nan_sequence(run, tol=1e-6):
    """rhs; mg_outer(tol); run_cycles(2) -> dict(outer, visits, its, u)."""
    run.rhs()
    outer = run.mg_outer(tol)
    run.cycle()
    run.cycle()
    return dict(outer=outer, visits=list(run.visits), its=run.coarse_its, u=run.u.copy())

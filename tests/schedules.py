"""The schedules below the default one, as a list of cases that the CPU margin
file (tests/test_schedules_fields.py) and the GPU file
(tests/test_gpu_schedules.py) share (numpy only, in the style of tests/bdf.py).

A case is (N, L, params, field, tower, fp, nsmooth, fuse, shape, form, parts,
tol): params a name of fields.PARAMS, field one of fields.make, tower 0 / 1 =
reference / correct, fp 0 / 1 = bitwise / fma, shape 1 / 2 = V / W, parts > 0 =
that many virtual ranks, tol the tolerance of its mg_outer and steps.  `form`
names the tuning keys that fix which kernel the level passes run as (FORMS):

  "tiles"  tile_max_n = 2048: every level of every case here (N <= 2048) is a
           pass of 2-D LDS tiles (k_smooth_tile), the finest included.
  "march"  tile_max_n = 0 and march_tile_rows = 0: every level is the
           wave-private row march (k_wsmooth).  With both keys 0
           smooth_as_tiles (csrc/wsmooth.hip) has no tile branch left -- `n <=
           tile_max_n` is false for every n >= 1 and `groups * rows < slots *
           march_tile_rows` is `... < 0` -- and smooth_block only ever launches
           tiles where smooth_as_tiles says so: it never falls back from a
           march to tiles.  That is the proof for level 0, which has no
           observable of its own; levels >= 1 also show it through the packed
           form (wpack), which exists on a march only.
  "mixed"  tile_max_n = N / 4 and march_tile_rows = 0: levels 0 and 1 march,
           levels >= 2 are tiles; the first tile level sits right under a
           march level, and takes the fused coarsest solve only where it is
           the level above the coarsest (L = 4).

The list is hand-picked, not the product.  check_coverage() states what it must
keep covering, and tests/test_schedules_fields.py asserts it, so a later edit
cannot thin it silently: every value of nsmooth, fuse, tower, fp and field with
every shape and with every form; fuse < nsmooth and nsmooth 4 with fuse 3 (3 +
1 sweeps); and per shape every form of the coarsest solve -- n = 2 and 4 (L = 8
and 7 at N = 256), 32 and 64 (LDS; fused into the tile pass above it), 128 (one
workgroup, u in L2), 512 (the host loop) -- plus L = 1 (the finest level is the
coarsest) and L = 2.  Three cases run on two virtual ranks at N = 1024 (a
W-cycle, nsmooth 4, nsmooth 1; dist_min_rows at its default).  The N = 4096
W-cycle case, L = 7, lives in tests/test_gpu_generic_fields.py (cycles_case),
where it shares that module's cached fields.

params and tol are chosen per case so that the checker alone converges under
the cycle cap with every r_k / r_0 at least fields.MARGIN from tol (the figures
are in tests/test_schedules_fields.py): three cycles run before the mg_outer,
so a schedule that contracts by 1e-4 a cycle has reached the rounding floor by
then and needs a thinner viscosity, and one that contracts by 0.5 needs the
easy time step.

fp_mode fma contracts the fused smoothing passes and the coarsest solve only;
the stand-alone residual kernels (mgx_residual_norm, mgx_restrict) keep the
reference's expressions in both modes (include/mgx.h), while the checker's fma
mode contracts every residual (oracle/mg_oracle.h).  The two agree wherever the
norm and the restriction are stages of a smoothing pass, that is with L >= 2
and nsmooth >= 1; the L = 1 and nsmooth = 0 cases, whose norm and restriction
are the stand-alone kernels, are therefore bitwise-mode cases (in fma mode the
solver is within rounding of the checker there -- measured 2e-15 in u, 5e-9
relative in a norm of 1e-6 -- but not equal to it).

The sequence of every case, on the checker (checker_sequence) and on the solver
(solver_sequence) alike: rhs; run_cycles(1) twice; one op-level mg_inner;
download; mg_outer(tol); download; two step_ex(tol); download.  nsmooth = 0
cases stop after the mg_inner's download: nothing converges there.
"""
import collections

import fields as F

Case = collections.namedtuple(
    "Case", "N L params field tower fp nsmooth fuse shape form parts tol")

FORMS = ("tiles", "march", "mixed")


def form_keys(form, N):
    """The tuning keys of a form at finest size N."""
    return {"tiles": dict(tile_max_n=2048),
            "march": dict(tile_max_n=0, march_tile_rows=0),
            "mixed": dict(tile_max_n=N // 4, march_tile_rows=0)}[form]


def level_forms(case):
    """-> per level 0 .. L-2 "tiles" or "march" (the coarsest level is a solve)."""
    tmax = form_keys(case.form, case.N)["tile_max_n"]
    return ["tiles" if (case.N >> l) <= tmax else "march" for l in range(case.L - 1)]


def coarsest_n(case):
    return case.N >> (case.L - 1)


REF, COR = 0, 1
BIT, FMA = 0, 1
V, W = 1, 2


def _c(N, L, params, field, tower, fp, nsmooth, fuse, shape, form, tol, parts=0):
    return Case(N, L, params, field, tower, fp, nsmooth, fuse, shape, form, parts, tol)


CASES = [
    # ---- N = 128: L = 1 (coarsest n = 128, one workgroup), L = 2 (64), L = 3 (32)
    _c(128, 1, "easy5", "generic", REF, BIT, 3, 3, V, "tiles", 1e-6),
    _c(128, 1, "visc16", "generic0", COR, BIT, 2, 2, W, "march", 1e-6),
    _c(128, 2, "visc07", "generic", REF, FMA, 3, 3, W, "tiles", 1e-6),
    _c(128, 2, "easy3", "rank1", COR, BIT, 1, 1, V, "march", 1e-6),
    _c(128, 3, "visc07", "generic", REF, BIT, 3, 3, W, "tiles", 1e-6),
    _c(128, 3, "visc16", "generic", REF, FMA, 2, 1, V, "tiles", 1e-6),
    _c(128, 3, "visc16", "generic0", REF, BIT, 0, 3, V, "march", 1e-6),
    _c(128, 3, "visc06", "rank1", COR, FMA, 1, 3, W, "march", 1e-9),
    _c(128, 3, "visc07", "generic", COR, BIT, 4, 3, V, "tiles", 1e-6),
    _c(128, 3, "visc16", "generic", REF, BIT, 0, 1, W, "tiles", 1e-6),
    # ---- N = 256: L = 8 and 7 (coarsest n = 2 and 4), 4 (32), 3 (64), 2 (128)
    _c(256, 8, "visc16", "generic", REF, BIT, 3, 3, V, "tiles", 1e-6),
    _c(256, 8, "visc16", "rank1", COR, FMA, 2, 2, W, "march", 1e-9),
    _c(256, 8, "visc16", "generic0", REF, FMA, 2, 3, V, "mixed", 1e-6),
    _c(256, 7, "visc16", "generic", COR, BIT, 3, 3, W, "tiles", 1e-6),
    _c(256, 7, "easy3", "generic", REF, FMA, 1, 1, V, "mixed", 1e-6),
    _c(256, 7, "visc16", "generic", REF, BIT, 3, 2, W, "mixed", 1e-6),
    _c(256, 4, "visc30", "generic", REF, FMA, 3, 3, W, "mixed", 1e-9),
    _c(256, 4, "visc16", "generic", COR, FMA, 3, 3, V, "mixed", 1e-6),
    _c(256, 4, "visc06", "generic0", REF, BIT, 4, 3, W, "tiles", 1e-6),
    _c(256, 4, "visc16", "rank1", REF, BIT, 2, 2, V, "march", 1e-6),
    _c(256, 4, "visc16", "generic", REF, BIT, 0, 2, V, "mixed", 1e-6),
    _c(256, 3, "visc16", "generic", REF, BIT, 3, 3, V, "march", 1e-6),
    _c(256, 3, "visc16", "generic", COR, FMA, 2, 2, W, "tiles", 1e-6),
    _c(256, 3, "visc30", "rank1", REF, FMA, 4, 3, W, "march", 1e-9),
    _c(256, 2, "visc16", "generic", REF, FMA, 3, 1, V, "tiles", 1e-6),
    _c(256, 2, "visc07", "generic0", COR, BIT, 3, 3, W, "march", 1e-6),
    # ---- N = 512: L = 5 (32), 4 (64), 3 (128); "mixed": 512 and 256 march
    _c(512, 5, "visc07", "generic", REF, BIT, 3, 3, W, "march", 1e-6),
    _c(512, 5, "visc16", "generic", REF, FMA, 3, 3, V, "tiles", 1e-6),
    _c(512, 5, "easy3", "generic0", COR, BIT, 1, 2, W, "mixed", 1e-6),
    _c(512, 5, "visc16", "rank1", REF, FMA, 4, 3, V, "mixed", 1e-9),
    _c(512, 5, "visc16", "generic", COR, BIT, 0, 3, W, "march", 1e-6),
    _c(512, 4, "visc30", "rank1", COR, BIT, 3, 3, W, "mixed", 1e-9),
    _c(512, 4, "easy3", "generic", REF, FMA, 2, 2, V, "march", 1e-6),
    _c(512, 4, "visc16", "generic", REF, BIT, 2, 1, W, "tiles", 1e-6),
    _c(512, 4, "easy5", "generic", REF, FMA, 1, 1, V, "tiles", 1e-9),
    _c(512, 4, "visc16", "rank1", REF, BIT, 0, 3, V, "tiles", 1e-6),
    _c(512, 3, "visc16", "generic", REF, BIT, 3, 3, V, "tiles", 1e-6),
    _c(512, 3, "visc07", "generic", REF, FMA, 2, 3, W, "march", 1e-6),
    _c(512, 3, "easy3", "generic0", COR, FMA, 1, 3, W, "tiles", 1e-6),
    _c(512, 3, "visc07", "generic", COR, BIT, 4, 3, V, "march", 1e-6),
    # ---- N = 2048: L = 3 (coarsest n = 512: the host loop); the smallest level
    # that marches by default
    _c(2048, 3, "stiff", "generic", REF, FMA, 3, 3, V, "march", 1e-9),
    _c(2048, 3, "visc07", "generic", REF, BIT, 3, 3, W, "tiles", 1e-6),
    _c(2048, 6, "stiff", "generic", COR, FMA, 2, 2, W, "mixed", 1e-6),
    _c(2048, 6, "visc16", "rank1", REF, BIT, 4, 3, V, "mixed", 1e-6),
    # ---- two virtual ranks at N = 1024 (dist_min_rows at its default)
    _c(1024, 5, "visc07", "generic", REF, FMA, 3, 3, W, "tiles", 1e-6, parts=2),
    _c(1024, 5, "visc07", "generic", REF, BIT, 4, 3, V, "mixed", 1e-6, parts=2),
    _c(1024, 5, "easy5", "generic", COR, FMA, 1, 1, V, "march", 1e-6, parts=2),
]


def case_id(c):
    return "N%d-L%d-%s-%s-t%d-%s-s%df%d-%s-%s%s" % (
        c.N, c.L, c.params, c.field, c.tower, "fma" if c.fp else "bitwise", c.nsmooth, c.fuse,
        "W" if c.shape == 2 else "V", c.form, "-p%d" % c.parts if c.parts else "")


CASE_IDS = [case_id(c) for c in CASES]

# what the list must keep covering (check_coverage)
AXES = {"nsmooth": (0, 1, 2, 3, 4), "fuse": (1, 2, 3), "tower": (REF, COR), "fp": (BIT, FMA),
        "field": ("generic", "generic0", "rank1")}
COARSEST_N = (2, 4, 32, 64, 128, 512)


def check_coverage(cases=None):
    """-> the list of what `cases` (CASES) no longer covers; empty = all there."""
    cases = CASES if cases is None else cases
    missing = []
    for axis, values in AXES.items():
        for v in values:
            for shape in (V, W):
                if not any(getattr(c, axis) == v and c.shape == shape for c in cases):
                    missing.append((axis, v, "shape", shape))
            for form in FORMS:
                if not any(getattr(c, axis) == v and c.form == form for c in cases):
                    missing.append((axis, v, "form", form))
    for shape in (V, W):
        for form in FORMS:
            if not any(c.shape == shape and c.form == form for c in cases):
                missing.append(("shape", shape, "form", form))
        for n in COARSEST_N:
            if not any(coarsest_n(c) == n and c.shape == shape for c in cases):
                missing.append(("coarsest n", n, "shape", shape))
        for L in (1, 2):
            if not any(c.L == L and c.shape == shape for c in cases):
                missing.append(("L", L, "shape", shape))
    if not any(c.fuse < c.nsmooth and c.nsmooth in (2, 3) for c in cases):
        missing.append("fuse < nsmooth")
    if not any(c.nsmooth == 2 and c.fuse == 1 for c in cases):
        missing.append("nsmooth 2, fuse 1")
    if not any(c.nsmooth == 4 and c.fuse == 3 for c in cases):
        missing.append("nsmooth 4, fuse 3")
    if not any((c.N, c.L) == (256, 8) for c in cases) or \
            not any((c.N, c.L) == (256, 7) for c in cases) or \
            not any((c.N, c.L) == (2048, 3) for c in cases):
        missing.append("N=256 L=8 / L=7, N=2048 L=3")
    dist = [c for c in cases if c.parts]
    if len(dist) < 3 or any((c.N, c.parts) != (1024, 2) for c in dist) or \
            not any(c.shape == W for c in dist) or \
            not any(c.nsmooth == 4 for c in dist) or not any(c.nsmooth == 1 for c in dist):
        missing.append("parts=2 at N=1024: a W-cycle, nsmooth 4, nsmooth 1")
    return missing


def converges(case):
    """Does the case run mg_outer and the steps?"""
    return case.nsmooth > 0


def checker_run(O, case, u0, v1, v2):
    """A fields.CheckerRun of the case (the caller sets the checker's fp mode
    and threads, and closes the run)."""
    dt, nu = F.params(case.params, case.N)
    return F.CheckerRun(O, u0, v1, v2, case.N, case.L, dt, nu, case.tower, case.nsmooth,
                        case.shape, case.fp)


def checker_sequence(run, case):
    """The sequence on a fields.CheckerRun -> dict: norms (of the two
    run_cycles), its2 and its3 (coarsest-solve sweeps so far, before and after the
    mg_inner), u3, and for converging
    cases outer = (cycles, r0, [r_k]), uo, steps = [(cycles, r0, [r_k])] x 2,
    us, its."""
    out = {}
    run.rhs()
    out["norms"] = [run.cycle(), run.cycle()]
    out["its2"] = run.coarse_its
    run.mg_inner()
    out["u3"] = run.u.copy()
    out["its3"] = run.coarse_its
    if converges(case):
        out["outer"] = run.mg_outer(case.tol)
        out["uo"] = run.u.copy()
        out["steps"] = [run.step(case.tol) for _ in range(2)]
        out["us"] = run.u.copy()
        out["its"] = run.coarse_its
    return out


def solver_sequence(mg, case, u0, v1, v2, around_inner=None):
    """The sequence on a Multigrid (the fields uploaded here) -> dict: norms,
    its2, u3, its3, and for converging cases outer = (cycles, r0, r, capped), uo, steps =
    [(cycles, r0, r)] x 2, us, its.  around_inner: a context manager entered
    around the op-level mg_inner alone (the GPU file profiles that one cycle)."""
    out = {}
    mg.upload(u0, v1, v2)
    mg.rhs()
    out["norms"] = [mg.run_cycles(1), mg.run_cycles(1)]
    out["its2"] = mg.coarse_iterations()
    if around_inner is None:
        mg.mg_inner()
    else:
        with around_inner:
            mg.mg_inner()
    out["u3"] = mg.download()
    out["its3"] = mg.coarse_iterations()
    if converges(case):
        out["outer"] = mg.mg_outer(case.tol)
        out["uo"] = mg.download()
        out["steps"] = [mg.step_ex(case.tol) for _ in range(2)]
        out["us"] = mg.download()
        out["its"] = mg.coarse_iterations()
    return out


def outers(want):
    """The (r0, norms) of every mg_outer of a checker_sequence result."""
    return [(want["outer"][1], want["outer"][2])] + [(s[1], s[2]) for s in want["steps"]]

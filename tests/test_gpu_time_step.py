"""Per-step dt and theta on a live context (mgx_set_time_step, csrc/tstep.hip)
against the CPU checker and against the calls that define it.

Meaning.  A step (m, theta) is compute_rhs with k = kB, the source term, a
pending ring, then mg_outer with k = kA -- tsteps.checker_steps on the checker.
Bar: u after every step equals the checker's as uint64, the cycle counts are
equal, res0 and res agree with the accurately summed norms of the checker's
residuals (fields.Norm.exact) to 1e-11 relative, the bound include/mgx.h
documents.  Before a cycle count is compared the checker's own norms must be at
least 1 % away from the tolerance (fields.margin); tests/
test_time_step_fields.py holds the same condition on the CPU alone, with the
figures.

Sizes: N=8 (L=2) and 32 are single-strip grids with a partial last pair, N=128
runs the LDS-tile path, N=1024 two strips of the row march, N=4096 is the
smallest size with the cross-cycle pass, step fusion and velocity factors,
N=8192 with L=8 the smallest with the cross pass in step mode.  Every checker
run happens once per module and is shared by the tests that need it.
"""
import numpy as np
import pytest

import fields as F
import rings as R
import tsteps as T
from hpcclassmultigridproject_amd import Multigrid, _lib, dist

pytestmark = pytest.mark.gpu
NORM_RTOL = 1e-11
TOL = T.TOL
REF, CORRECT = _lib.TOWER_REFERENCE, _lib.TOWER_CORRECT
BITWISE, FMA = _lib.FP_BITWISE, _lib.FP_FMA

_FIELDS = {}
_CHECKER = {}
_SOLVER = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _FIELDS.clear()
    _CHECKER.clear()
    _SOLVER.clear()


def field(name, N):
    if (name, N) not in _FIELDS:
        arrs = F.make(name, N, F.SEED)
        for a in arrs:
            a.setflags(write=False)
        _FIELDS[name, N] = arrs
    return _FIELDS[name, N]


def with_checker(O, fp, fn):
    O.set_threads(16)
    O.set_fp_mode(fp)
    try:
        return fn()
    finally:
        O.set_fp_mode(0)
        O.set_threads(1)


def checker(O, N, L, pname, name, tower=REF, fp=BITWISE, seq=T.SEQ_EASY, extra=False,
            sched=T.SCHEDULE):
    """tsteps.checker_steps of one case, cached for the module; the margins of
    its norms are asserted before anything is compared with it."""
    key = (N, L, pname, name, tower, fp, seq, extra, sched)
    if key not in _CHECKER:
        dt, nu = F.params(pname, N)

        def go():
            run = F.CheckerRun(O, *field(name, N), N, L, dt, nu, tower, sched[0], sched[2], fp)
            try:
                return T.checker_steps(run, dt, seq, TOL, T.source_field(N)[2] if extra else None,
                                       T.RINGS if extra else None)
            finally:
                run.close()
        _CHECKER[key] = with_checker(O, fp, go)
    steps = _CHECKER[key]
    for cyc, r0, norms, _ in steps:
        assert cyc < 50 and norms[-1] / r0 <= TOL, (key, cyc, r0, norms)
        assert F.margin(r0, norms, TOL) >= F.MARGIN, (key, r0, norms)
    return steps


def solver(N, L, pname, name, tower=REF, fp=BITWISE, seq=T.SEQ_EASY, extra=False, sched=T.SCHEDULE):
    """tsteps.solver_steps of a fresh single-GPU context, cached."""
    key = (N, L, pname, name, tower, fp, seq, extra, sched)
    if key not in _SOLVER:
        dt, nu = F.params(pname, N)
        with Multigrid(N, L, dt, nu, nsmooth=sched[0], fuse=sched[1], shape=sched[2],
                       tower_mode=tower, fp_mode=fp) as mg:
            mg.upload(*field(name, N))
            if extra:
                a, b, _ = T.source_field(N)
                mg.set_source_separable(a, b)
            _SOLVER[key] = T.solver_steps(mg, dt, seq, TOL, T.RINGS if extra else None, N)
    return _SOLVER[key]


def bits_equal(got, want, N, what):
    g, w = got.view(np.uint64), want.view(np.uint64)
    if np.array_equal(g, w):
        return
    bad = (g.ravel() != w.ravel()).reshape(N + 1, N + 1)
    rows, cols = np.nonzero(bad)
    raise AssertionError(
        f"{what}: {bad.sum()} of {bad.size} entries differ, rows {rows.min()}..{rows.max()}, "
        f"columns {cols.min()}..{cols.max()}, first at ({rows[0]}, {cols[0]})")


def norm_close(got, want, what):
    rel = abs(got - want.exact) / abs(want.exact)
    print(f"{what}: got {got!r} checker {want.exact!r} rel {rel:.3e}")
    assert rel <= NORM_RTOL, (what, got, want.exact, rel)


def against_checker(got, want, N, what):
    assert len(got) == len(want)
    for k, ((cyc, r0, r, u), (ccyc, cr0, cnorms, cu)) in enumerate(zip(got, want)):
        assert cyc == ccyc, (what, k, cyc, ccyc)
        bits_equal(u, cu, N, f"{what} step {k}")
        norm_close(r0, cr0, f"{what} step {k} res0")
        norm_close(r, cnorms[-1], f"{what} step {k} res")


def same_steps(a, b, N, what):
    assert [s[0] for s in a] == [s[0] for s in b], what
    for k, (x, y) in enumerate(zip(a, b)):
        bits_equal(x[3], y[3], N, f"{what} step {k}")
        assert abs(x[1] - y[1]) <= NORM_RTOL * y[1] and abs(x[2] - y[2]) <= NORM_RTOL * y[2], (
            what, k, x[1:3], y[1:3])


@pytest.fixture
def knobs():
    """Set tuning keys for one test; restores the previous values."""
    saved = {}

    def set_(**kv):
        for k, v in kv.items():
            saved.setdefault(k, _lib.get_tuning(k))
            _lib.set_tuning(k, v)
    yield set_
    for k, v in saved.items():
        _lib.set_tuning(k, v)


# ---------------------------------------------------------------- 1. meaning
@pytest.mark.parametrize(T.CASE_ARGS, T.CASE_PARAMS, ids=T.CASE_IDS)
def test_steps_equal_the_checker(oracle_mod, N, L, pname, name, tower, fp, seq, extra, nsmooth,
                                 fuse, shape):
    sched = (nsmooth, fuse, shape)
    want = checker(oracle_mod, N, L, pname, name, tower, fp, seq, extra, sched)
    got = solver(N, L, pname, name, tower, fp, seq, extra, sched)
    against_checker(got, want, N, f"N={N} L={L} {pname} {name} tower={tower} fp={fp}")


# ---------------------------------------------------------------- 2. the pass
def sources(N):
    """-> {kind: (setter args, f flat or None)}: no source, a field, separable
    sources of one and of four terms (f in the order include/mgx.h states)."""
    rng = np.random.default_rng(500 + N)
    w = N + 1
    fld = rng.standard_normal(w * w)
    a = rng.uniform(-2, 2, (4, w))
    b = rng.uniform(-2, 2, (4, w))
    f1 = a[0][:, None] * b[0][None, :]
    f4 = f1
    for r in range(1, 4):
        f4 = f4 + a[r][:, None] * b[r][None, :]
    return {"none": (None, None), "field": (("field", fld), fld),
            "sep1": (("sep", a[0].copy(), b[0].copy()), f1.ravel()),
            "sep4": (("sep", a, b), f4.ravel())}


def set_src(mg, spec):
    if spec is None:
        mg.set_source(None)
    elif spec[0] == "field":
        mg.set_source(spec[1])
    else:
        mg.set_source_separable(spec[1], spec[2])


@pytest.mark.parametrize("name", ["generic", "rank1"])
@pytest.mark.parametrize("N,L", [(8, 2), (32, 3), (128, 3), (1024, 6), (4096, 7)])
def test_the_pass_equals_rhs_then_residual_norm(oracle_mod, knobs, N, L, name):
    """step_ex's first pass against mgx_rhs + mgx_residual_norm(0) on a twin
    context, and its rhs against the checker's compute_rhs with k = kB."""
    O = oracle_mod
    dt, nu = F.params("easy", N)
    u0, v1, v2 = field(name, N)
    w = N + 1
    srcs = sources(N)
    with Multigrid(N, L, dt, nu, fp_mode=FMA) as mg, Multigrid(N, L, dt, nu, fp_mode=FMA) as twin:
        twin.upload(u0, v1, v2)
        if name == "rank1" and N >= 4096:
            assert twin.velocity_factored() & 1    # the factor instantiations run
        for theta in (1, .75):
            kA, kB = T.k_pair(dt, theta)
            assert kA != kB
            base = with_checker(O, 0, lambda: O.compute_rhs(np.array(u0), N, np.array(v1),
                                                            np.array(v2), float(kB), nu, 1.0 / N))
            for kind, (spec, f) in srcs.items():
                want = base
                if f is not None:
                    want = base.copy().reshape(w, w)
                    want[1:N, 1:N] = (base.reshape(w, w) + np.float64(dt) * f.reshape(w, w))[1:N, 1:N]
                    want = want.ravel()
                for sv in (1, 0):
                    knobs(source_sv=sv)
                    what = f"N={N} {name} theta={theta} {kind} source_sv={sv}"
                    mg.upload(u0, v1, v2)
                    for m in (mg, twin):
                        set_src(m, spec)
                        m.set_time_step(dt, theta)
                    mg.profile(True)
                    _, res0, _ = mg.step_ex(.5)
                    n_rhs, _, bytes_, cbytes = mg.profile_get_ex(_lib.K_RHS, 0)
                    mg.profile(False)
                    mg.profile_reset()
                    twin.rhs()
                    r = twin.residual_norm(0)
                    print(f"{what}: res0 {res0!r} twin {r!r}")
                    assert res0 == r, (what, res0, r)
                    got = mg.download_level(0, "rhs")
                    bits_equal(got, twin.download_level(0, "rhs"), N, what + ": rhs against mgx_rhs")
                    bits_equal(got, want, N, what + ": rhs against the checker")
                    # one launch; the accounting include/mgx.h states
                    M = float(w * w)
                    fac = bool(sv and mg.velocity_factored() & 1)
                    fs = kind == "field"
                    assert n_rhs == 1, (what, n_rhs)
                    assert bytes_ == (88.0 if fs else 80.0) * M, (what, bytes_)
                    assert cbytes == ((16.0 if fac else 32.0) + (8.0 if fs else 0.0)) * M, (
                        what, cbytes)


# ---------------------------------------------------------------- 3. identity
def test_crank_nicolson_with_the_dt_of_create_changes_nothing():
    N, L, pname, name = 4096, 7, "easy", "generic"
    dt, nu = F.params(pname, N)
    seq = ((1, .5),) * 3
    runs = []
    for call in (False, True):
        with Multigrid(N, L, dt, nu, fp_mode=FMA) as mg:
            mg.upload(*field(name, N))
            steps = []
            for k in range(3):
                if call and k > 0:
                    mg.set_time_step(dt, .5)
                    assert mg.time_step() == (dt, .5)
                cyc, r0, r = mg.step_ex(TOL)
                steps.append((cyc, r0, r, mg.download()))
            runs.append(steps)
    assert len(seq) == 3
    for k, (a, b) in enumerate(zip(*runs)):
        assert a[0] == b[0], (k, a[0], b[0])
        bits_equal(b[3], a[3], N, f"identity step {k}")
        # (a step prepared by the cross pass takes its norms in that kernel)
        assert abs(a[1] - b[1]) <= NORM_RTOL * a[1] and abs(a[2] - b[2]) <= NORM_RTOL * a[2]


# ---------------------------------------------------------------- 4. what is dropped
def test_captured_subcycles_are_dropped(knobs):
    """graph_level: the nodes of a captured sub-cycle hold the old coefficients
    as kernel arguments; after a dt change the sub-cycle is captured again and
    the cycles equal the launched schedule's bit for bit."""
    N, L, gl = 1024, 5, 2
    dt, nu = F.params("easy", N)
    out = []
    for g in (0, gl):
        knobs(graph_level=g)
        with Multigrid(N, L, dt, nu, fp_mode=FMA) as mg:
            mg.upload(*field("generic", N))
            mg.rhs()
            na = mg.run_cycles(2)
            c0 = _lib.get_tuning("graph_captures")
            mg.set_time_step(3 * dt, 1.0)
            mg.rhs()
            nb = mg.run_cycles(2)
            mg.mg_inner()
            out.append((mg.download(), na, nb, _lib.get_tuning("graph_captures") - c0))
    (u0_, na0, nb0, cap0), (u1_, na1, nb1, cap1) = out
    assert cap0 == 0 and cap1 > 0, (cap0, cap1)
    assert (na0, nb0) == (na1, nb1)
    bits_equal(u1_, u0_, N, "graph_level against launches after a dt change")


def test_a_packed_u_pre_is_expanded_first(oracle_mod):
    """fma inside run_cycles: a packed u_pre is current (xpack 2).  The call
    expands it with the operator that packed it: u is the checker's after the
    two cycles, and the cycle after the change is the checker's with the new
    coefficients."""
    O = oracle_mod
    N, L = 4096, 7
    dt, nu = F.params("easy", N)
    assert _lib.get_tuning("xpack") in (1, 2)
    dt2, theta = float(np.float64(.5) * np.float64(dt)), 1.0
    kA, kB = T.k_pair(dt2, theta)

    def go():
        run = F.CheckerRun(O, *field("generic", N), N, L, dt, nu, REF, fp=FMA)
        try:
            run.rhs()
            run.cycle()
            run.cycle()
            ua = run.u.copy()
            run.dt = float(kB)
            run.rhs()
            run.dt = float(kA)
            run.cycle()
            return ua, run.u.copy()
        finally:
            run.close()
    ua, ub = with_checker(O, FMA, go)
    with Multigrid(N, L, dt, nu, fp_mode=FMA) as mg:
        mg.upload(*field("generic", N))
        mg.rhs()
        mg.run_cycles(2)
        mg.set_time_step(dt2, theta)
        bits_equal(mg.download(), ua, N, "u after the call")
        mg.rhs()
        mg.run_cycles(1)
        bits_equal(mg.download(), ub, N, "a cycle with the new coefficients")


# ---------------------------------------------------------------- 5. what stays
def test_the_setting_and_what_survives_it():
    N, L = 128, 3
    dt, nu = F.params("easy", N)
    u0, v1, v2 = field("generic", N)
    a, b, f = T.source_field(N)
    g = R.ring(N, 1)
    with Multigrid(N, L, dt, nu) as mg:
        assert mg.time_step() == (dt, .5) and (mg.dt, mg.theta) == (dt, .5)
        mg.upload(u0, v1, v2)
        mg.set_source(f)
        mg.set_source_scale(.25)
        mg.set_boundary(g, "next")
        cfl0 = mg.cfl()
        mg.set_time_step(2 * dt, .75)
        assert mg.time_step() == (2 * dt, .75) and (mg.dt, mg.theta) == (2 * dt, .75)
        assert mg.cfl() == 2 * cfl0   # (a power of two: exact)
        assert mg.source_info() == (True, .25)
        assert mg.boundary_pending() == 1
        mg.set_time_step(theta=1)              # None keeps the current value
        assert mg.time_step() == (2 * dt, 1.0)
        mg.set_time_step(dt=dt)
        assert mg.time_step() == (dt, 1.0)
        for bad in ((0.0, .5), (dt, 0.0), (dt, 1.5), (float("nan"), .5), (dt, float("nan"))):
            with pytest.raises(_lib.MGXError) as e:
                mg.set_time_step(*bad)
            assert e.value.code == _lib.MGX_E_ARG and "mgx_set_time_step" in str(e.value)
        assert mg.time_step() == (dt, 1.0) and (mg.dt, mg.theta) == (dt, 1.0)
        assert mg.boundary_pending() == 1 and mg.source_info() == (True, .25)
        # the setting belongs to the context: upload and set_velocity keep it
        mg.set_velocity(np.array(v2), np.array(v1))
        assert mg.time_step() == (dt, 1.0)
        mg.upload(u0, v1, v2)                  # (cancels the ring, keeps the source)
        assert mg.time_step() == (dt, 1.0) and mg.source_info() == (True, .25)
        # ... and it is what the next rhs uses: k = kB = 0 at theta = 1
        mg.set_source(None)
        mg.rhs()
        U = np.array(u0).reshape(N + 1, N + 1)
        got = mg.download_level(0, "rhs").reshape(N + 1, N + 1)
        assert np.array_equal(got[1:N, 1:N], U[1:N, 1:N])


# ---------------------------------------------------------------- 6. step fusions
def test_step_fusions_resume_at_crank_nicolson(knobs):
    """N=8192, L=8: the same bits and cycle counts with step_cross / step_fuse 1
    and 0; with 1 the third step (the same setting as the second: no call in
    between, a call would drop it) starts from the state the second prepared,
    one MGX_K_RHS launch less.

    A step is prepared by the cycle mg_outer predicts to be its last.  With the
    default post_only = 10 no step of this sequence is both predicted and kept:
    the first one's is dropped by the dt change, and the 3-cycle steps at 2 dt0
    end too close to the tolerance to be predicted (checker, N=8192 fma, r_k /
    r_0 of step 2: 2.2e-4, 2.7e-7, 4.0e-10 -- extrapolated from the first two
    3.2e-10, not within tol / 10), measured: 5 launches either way.  post_only
    = -1 (every cycle runs as if it were the last; the key's documented test
    setting) takes the predictor out of the question for both runs."""
    N, L = 8192, 8
    dt, nu = F.params("easy", N)
    runs = []
    knobs(post_only=-1)
    for on in (1, 0):
        knobs(step_cross=on, step_fuse=on)
        with Multigrid(N, L, dt, nu, fp_mode=FMA) as mg:
            mg.upload(*field("generic", N))
            mg.profile(True)
            steps, prev = [], T.SEQ_FUSE[0]
            for m, theta in T.SEQ_FUSE:
                if (m, theta) != prev:
                    mg.set_time_step(float(np.float64(m) * np.float64(dt)), theta)
                prev = (m, theta)
                cyc, r0, r = mg.step_ex(TOL)
                steps.append((cyc, r0, r, mg.download()))
            n_rhs = mg.profile_get(_lib.K_RHS)[0]
            mg.profile(False)
            runs.append((steps, n_rhs))
    (s1, n1), (s0, n0) = runs
    print("cycles", [s[0] for s in s1], "K_RHS launches", n1, n0)
    assert n0 == len(T.SEQ_FUSE) and n1 < n0, (n1, n0)
    same_steps(s1, s0, N, "step fusions 1 against 0")


# ---------------------------------------------------------------- 7. partitioned contexts
def run_partitioned(N, L, make_ctx, upload):
    dt, nu = F.params("easy", N)
    with make_ctx(dt, nu) as mg:
        upload(mg)
        steps = T.solver_steps(mg, dt, T.SEQ_EASY, TOL)
        assert mg.time_step() == (dt, .5)
    return steps


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("N,L,min_rows", [(1024, 6, 16), (4096, 6, 256), (256, 4, 256)],
                         ids=["N1024", "N4096", "N256-replicated"])
def test_local_parts_equal_single(oracle_mod, knobs, N, L, min_rows, G):
    checker(oracle_mod, N, L, "easy", "generic", fp=FMA)   # (the margins)
    knobs(dist_min_rows=min_rows)

    def make(dt, nu):
        mg = Multigrid(N, L, dt, nu, fp_mode=FMA, local_parts=G)
        assert (mg.dist_info()[2] == 0) == (N == 256)   # every level replicated at N=256
        return mg
    got = run_partitioned(N, L, make, lambda mg: mg.upload(*field("generic", N)))
    same_steps(got, solver(N, L, "easy", "generic", fp=FMA), N, f"N={N} G={G}")


def test_row_block_upload_equals_single(oracle_mod, knobs):
    """A context no host holds u of: filled by upload_rows (correct tower)."""
    N, L, G = 1024, 6, 2
    checker(oracle_mod, N, L, "easy", "generic", tower=CORRECT, fp=FMA)
    knobs(dist_min_rows=16)
    w = N + 1

    def upload(mg):
        blocks = []
        for part in range(G):
            lo, hi = mg.dist_rows(part)
            blocks.append(tuple(np.ascontiguousarray(a.reshape(w, w)[lo:hi + 1]).ravel()
                                for a in field("generic", N)))
        mg.upload_rows(blocks)
    got = run_partitioned(
        N, L, lambda dt, nu: Multigrid(N, L, dt, nu, fp_mode=FMA, tower_mode=CORRECT,
                                       local_parts=G), upload)
    same_steps(got, solver(N, L, "easy", "generic", tower=CORRECT, fp=FMA), N, "upload_rows")


def test_rccl_world1_equals_single(oracle_mod):
    """The RCCL code path on a size-1 communicator."""
    N, L = 1024, 6
    checker(oracle_mod, N, L, "easy", "generic", fp=FMA)
    uid = dist.unique_id()
    got = run_partitioned(
        N, L, lambda dt, nu: Multigrid(N, L, dt, nu, fp_mode=FMA, world=1, rank=0, unique_id=uid),
        lambda mg: mg.upload(*field("generic", N)))
    same_steps(got, solver(N, L, "easy", "generic", fp=FMA), N, "rccl world 1")


# ---------------------------------------------------------------- 8. a W-cycle context
@pytest.mark.parametrize("graph_level", [0, 1])
def test_w_cycle_set_velocity_between_steps(oracle_mod, knobs, graph_level):
    """tsteps.CASES' W-cycle context (N=256, L=4: pair passes, the coarsest
    solve deferred into them) takes a step, then set_velocity with the two
    arrays swapped, then another step: the second equals a checker tower
    rebuilt with that velocity from the downloaded u."""
    O = oracle_mod
    N, L, sched = 256, 4, (3, 3, 2)
    dt, nu = F.params("easy", N)
    u0, v1, v2 = field("generic", N)

    def one_step(u, a, b):
        def go():
            run = F.CheckerRun(O, u, a, b, N, L, dt, nu, REF, sched[0], sched[2], FMA)
            try:
                return T.checker_steps(run, dt, ((1, .5),), TOL)
            finally:
                run.close()
        steps = with_checker(O, FMA, go)
        for cyc, r0, norms, _ in steps:
            assert cyc < 50 and norms[-1] / r0 <= TOL, (cyc, r0, norms)
            assert F.margin(r0, norms, TOL) >= F.MARGIN, (r0, norms)
        return steps
    knobs(graph_level=graph_level)
    assert _lib.get_tuning("graph_level") == graph_level
    c0 = _lib.get_tuning("graph_captures")
    with Multigrid(N, L, dt, nu, nsmooth=sched[0], fuse=sched[1], shape=sched[2],
                   fp_mode=FMA) as mg:
        mg.upload(u0, v1, v2)
        cyc, r0, r = mg.step_ex(TOL)
        u1 = mg.download()
        against_checker([(cyc, r0, r, u1)], one_step(u0, v1, v2), N, "first step")
        mg.set_velocity(np.array(v2), np.array(v1))
        want = one_step(u1, np.array(v2), np.array(v1))
        cyc, r0, r = mg.step_ex(TOL)
        against_checker([(cyc, r0, r, mg.download())], want, N, "step after set_velocity")
    # (level 1's sub-cycle went through the graph path: a W-cycle enters it twice
    # a cycle, from different states, and these steps take one cycle each)
    c1 = _lib.get_tuning("graph_captures")
    assert (c1 > c0) if graph_level else (c1 == c0), (c0, c1)

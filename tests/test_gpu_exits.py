"""GPU: the solver's exits against the CPU checker -- the cycle cap of mg_outer
and of the steps, the limits of the coarsest solve in each of its forms, the
range of the fused passes' division, and a NaN (tests/exits.py holds the cases,
the checker sequences and the checker's figures; tests/test_exits_fields.py
asserts on the checker alone the conditions the comparisons here rest on).

Cycle cap.  u as uint64 equals the checker's after exactly min(max_cycle, c*)
cycles (c* the checker's own count), `cycles` is the checker's, capped ==
(cycles == max_cycle) -- also where that last allowed cycle reached the
tolerance, MGX_E_NOCONV all the same -- and r0, r agree with fields.Norm.exact
to 1e-11.  A second mg_outer on the same context with nothing in between then
equals the checker continuing from that state (under the same cap: it is the
context's): the dropped speculative state, a packed u_pre and the coarse levels
are consistent after a capped return.  Observables: the tuning keys read back,
the cross pass ran (or not: cross_cycle 0, N = 512), dist_info, the K_RHS and
finest K_GS launch counts of the steps.

Steps at N = 8192 (slow), step_cross 1, two step_ex, K_RHS launches on level 0:
  max_cycle 1  2: each step's only cycle is the last allowed one, so it runs the
               step-mode cross pass, which forms the next step's rhs, norm and
               pre-smoothing -- and is dropped, the cycle not having converged
               (8.6e-6 > 1e-9): the second step makes its own rhs + norm pass.
  max_cycle 2  1: the step converges on its last allowed cycle (capped, r / r0
               <= tol), the prepared step is kept, the second step consumes it.

Coarsest solve.  rhs, then run_cycles(1) twice: u bitwise, coarse_iterations()
after each call equal to the checker's running count, norms to 1e-11, for the
six limits of exits.limits on every form of exits.COARSE_FORMS.  Observables:
K_COARSE launches (none where the solve is fused into the tile pass above it or
loops on the host, one per cycle and entry else -- each `shape` solves), K_GS
launches on the coarsest level equal to the sweep count on the host loop,
graph_captures / graph_replays, dist_info.  coarse_lds has none: the key reads
back.

Division.  The level-pass sequence of tests/test_gpu_generic_fields.py
(seq_levels, "easy", L = 3) on generic() with u0 scaled by
2^-900 and 2^+400 -- bitwise, norms exact where the squares underflow to 0 --
and by 2^-1000, below the threshold of tests/test_division.py, where smoother
0's quotients may be one ulp off and smoother 1 (the true division) is bitwise.
Measured at 2^-1000 on an MI355X, entries that differ from the checker's by one
ulp (none by more), the same as tiles, as 32-row tiles and as the row march:
  N=128: u after gs(0, 3) 0 of 16641; u[1] after gs(1, 1) 94 of 4225 (2.2 %); u
         after prolong_add 0
  N=512: 1 of 263169; 565 of 66049 (0.86 %); 1 of 263169
(gs(0, 3)'s numerators are near 2^-1000, where a mismatch is one in millions;
level 1 smooths the residual, 2^-1015 and below: tests/test_division.py.)
The 151 tests of this file take 35 s on one MI355X, checker runs included; the
slowest, test_cycle_cap[1], 6.8 s, all of it the N = 4096 checker run that the
cycle-cap tests share; the two N = 8192 tests (slow) 6.1 and 2.8 s.
"""
import numpy as np
import pytest

import exits as E
import fields as F
import schedules as S
import test_gpu_generic_fields as G
import hpcclassmultigridproject_amd as pkg
from hpcclassmultigridproject_amd import Multigrid, _lib

pytestmark = pytest.mark.gpu
NORM_RTOL = 1e-11

_FIELDS = {}
_CHECKER = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _FIELDS.clear()
    _CHECKER.clear()


def field(name, N):
    if (name, N) not in _FIELDS:
        arrs = F.make(name, N)
        for a in arrs:
            a.setflags(write=False)
        _FIELDS[name, N] = arrs
    return _FIELDS[name, N]


def cached(O, key, fp, make):
    """make() with the checker in fp mode `fp` on 16 threads, once per key."""
    if key not in _CHECKER:
        O.set_threads(16)
        O.set_fp_mode(fp)
        try:
            _CHECKER[key] = make()
        finally:
            O.set_fp_mode(0)
            O.set_threads(1)
    return _CHECKER[key]


def closing(run, seq, *args):
    try:
        return seq(run, *args)
    finally:
        run.close()


@pytest.fixture
def knobs():
    saved = {}

    def set_(**kv):
        for k, v in kv.items():
            saved.setdefault(k, _lib.get_tuning(k))
            _lib.set_tuning(k, v)
            assert _lib.get_tuning(k) == v, k
    yield set_
    for k, v in saved.items():
        _lib.set_tuning(k, v)


bits_equal = G.bits_equal


def norms_close(got, want, what):
    want = np.array([w.exact for w in want])
    got = np.array(got)
    rel = np.abs(got - want) / np.abs(want)
    assert np.all(rel <= NORM_RTOL), (what, got.tolist(), want.tolist(), rel.tolist())


def margins_ok(outers, tol):
    for r0, norms in outers:
        assert F.margin(r0, norms, tol) >= F.MARGIN, (r0, norms, tol)


# ---------------------------------------------------------------- B. the cycle cap

def cap_want(O, case, caps):
    def make():
        want = closing(E.cap_run(O, case, *field(case.field, case.N)), E.cap_sequence, caps,
                       case.tol)
        margins_ok([(want["r0"], want["norms"])] +
                   [c["second"][1:] for c in want["caps"].values()], case.tol)
        return want
    return cached(O, ("cap", case, caps), case.fp, make)


def cap_case(O, knobs, case, caps, m, parts=0, expect_cross=True, **kv):
    """mg_outer under max_cycle = m and a second one, against the checker ->
    dist_info or None."""
    want = cap_want(O, case, caps)
    if case.shape == 1 and (m == 1 or kv.get("post_only") == -1):
        # every cycle is a post-only one (the only, hence last allowed, cycle;
        # or the key): no pass spans two cycles
        expect_cross = False
    if case.form:
        knobs(**S.form_keys(case.form, case.N))
    knobs(**kv)
    N, tol = case.N, case.tol
    dt, nu = F.params(case.params, N)
    c = want["caps"][m]
    with Multigrid(N, case.L, dt, nu, shape=case.shape, tower_mode=case.tower, fp_mode=case.fp,
                   max_cycle=m, local_parts=parts) as mg:
        assert mg.capped is None
        mg.upload(*field(case.field, N))
        mg.rhs()
        mg.profile(True, finest_only=True)
        cyc, r0, r, capped = mg.mg_outer(tol)
        assert cyc == c["first"] == min(m, len(want["norms"]))
        assert capped == (cyc == m) and mg.capped == capped
        norms_close([r0, r], [want["r0"], want["norms"][cyc - 1]], "the first mg_outer's norms")
        assert (r / r0 <= tol) == (want["norms"][cyc - 1] / want["r0"] <= tol)
        bits_equal(mg.download(), c["u1"], N, "u after mg_outer under max_cycle %d" % m)
        cyc2, r02, r2, capped2 = mg.mg_outer(tol)
        wc, wr0, wn = c["second"]
        assert cyc2 == wc
        assert capped2 == (cyc2 == m) and mg.capped == capped2
        norms_close([r02, r2], [wr0, wn[-1]], "the second mg_outer's norms")
        bits_equal(mg.download(), c["u2"], N, "u after the second mg_outer")
        x = mg.profile_get(_lib.K_XSMOOTH, 0)[0]
        mg.profile(False)
        assert (x > 0) == expect_cross, x
        return mg.dist_info() if parts else None


@pytest.mark.parametrize("m", E.CAP_MAIN_CAPS)
def test_cycle_cap(oracle_mod, knobs, m):
    """N = 4096, L = 5, generic, stiff, fma; c* = 6: max_cycle 6 converges on the
    last allowed cycle and is capped, 7 is not."""
    want = cap_want(oracle_mod, E.CAP_MAIN, E.CAP_MAIN_CAPS)
    assert len(want["norms"]) == 6 and want["norms"][-1] / want["r0"] <= E.TOL
    cap_case(oracle_mod, knobs, E.CAP_MAIN, E.CAP_MAIN_CAPS, m)


CAP_KNOBS = [
    ("post_predict_never", dict(post_predict=-1), {}),
    ("post_predict_always_store", dict(post_predict=0), {}),
    ("post_only_never", dict(post_only=0), {}),
    ("post_only_always", dict(post_only=-1), {}),
    ("cross_cycle0", dict(cross_cycle=0), dict(expect_cross=False)),
    ("xpack1", dict(xpack=1), {}),
    ("parts4", {}, dict(parts=4)),
    ("parts2_replicated", dict(dist_min_rows=8192), dict(parts=2)),
]


@pytest.mark.parametrize("m", E.CAP_KNOB_CAPS)
@pytest.mark.parametrize("kv,kw", [k[1:] for k in CAP_KNOBS], ids=[k[0] for k in CAP_KNOBS])
def test_cycle_cap_knobs(oracle_mod, knobs, kv, kw, m):
    """The same case against the one cached checker result under each knob."""
    info = cap_case(oracle_mod, knobs, E.CAP_MAIN, E.CAP_MAIN_CAPS, m, **kw, **kv)
    if kw.get("parts") == 4:
        assert info[0] == 4 and info[2] >= 1, info      # level 0 is partitioned
    if kw.get("parts") == 2:
        assert info[0] == 2 and info[2] == 0, info      # everything replicated


CAP_OTHER = [(c, caps, m) for c, caps in E.CAP_OTHER for m in caps]


@pytest.mark.parametrize("case,caps,m", CAP_OTHER,
                         ids=["%s-m%d" % (E.cap_id(c), m) for c, _, m in CAP_OTHER])
def test_cycle_cap_bitwise_mode_and_correct_tower(oracle_mod, knobs, case, caps, m):
    cap_case(oracle_mod, knobs, case, caps, m)


@pytest.mark.parametrize("m", E.CAP_W_CAPS)
def test_cycle_cap_w_cycle(oracle_mod, knobs, m):
    """W-cycles at L = 4 (the coarsest solve loops on the host), c* = 3."""
    want = cap_want(oracle_mod, E.CAP_W, E.CAP_W_CAPS)
    assert len(want["norms"]) == 3
    cap_case(oracle_mod, knobs, E.CAP_W, E.CAP_W_CAPS, m)


@pytest.mark.parametrize("case,caps", E.CAP_SMALL, ids=[E.cap_id(c) for c, _ in E.CAP_SMALL])
def test_cycle_cap_without_the_cross_pass(oracle_mod, knobs, case, caps):
    """N = 512: no third finest-level buffer, so no cross pass, no predicted
    store and no post-only cycle; as tiles and as the forced row march."""
    cap_case(oracle_mod, knobs, case, caps, caps[0], expect_cross=False)


def test_cycle_cap_growth(oracle_mod, knobs):
    """generic / stiff at N = 512 diverges: four cycles, each norm above the one
    before (tests/test_exits_fields.py), the call capped, u bitwise, and four
    more from there.  (op_mg_outer's predicted stores need the cross pass, N >=
    4096: test_cycle_cap_growth_with_the_cross_pass; here every cycle stores.)"""
    want = cap_want(oracle_mod, E.CAP_GROWTH, E.CAP_GROWTH_CAPS)
    seq = [want["r0"]] + want["norms"]
    assert all(b > a for a, b in zip(seq, seq[1:])) and np.all(np.isfinite(seq))
    cap_case(oracle_mod, knobs, E.CAP_GROWTH, E.CAP_GROWTH_CAPS, 4, expect_cross=False)


def test_cycle_cap_growth_with_the_cross_pass(oracle_mod, knobs):
    """N = 4096 with dt = 3 / N, nu = -2e-3: the norm falls for two cycles and
    grows from then on, so op_mg_outer's extrapolated norm r (r / r_prev) is
    formed with factors above 1 -- in the second call with nothing else.  No
    cycle but the last allowed one is predicted to converge (so none but that
    one stores its u_post), the calls end capped, u is bitwise."""
    case = E.CAP_GROWTH_CROSS
    want = cap_want(oracle_mod, case, E.CAP_GROWTH_CAPS)
    more = [want["caps"][4]["second"][1]] + want["caps"][4]["second"][2]
    assert want["norms"][3] > want["norms"][2] > want["norms"][1]
    assert all(b > a for a, b in zip(more, more[1:])) and np.all(np.isfinite(more))
    cap_case(oracle_mod, knobs, case, E.CAP_GROWTH_CAPS, 4)


def steps_want(O, case, steps, m):
    def make():
        want = closing(E.cap_run(O, case, *field(case.field, case.N)), E.cap_steps_sequence,
                       steps, m, case.tol)
        margins_ok([o[1:] for o in want["outers"]], case.tol)
        return want
    return cached(O, ("steps", case, steps, m), case.fp, make)


def steps_case(O, case, steps, m):
    """`steps` step_ex under max_cycle = m against the checker -> launches on
    level 0 {K_RHS, K_GS, K_XSMOOTH}."""
    want = steps_want(O, case, steps, m)
    N, tol = case.N, case.tol
    dt, nu = F.params(case.params, N)
    with Multigrid(N, case.L, dt, nu, tower_mode=case.tower, fp_mode=case.fp, max_cycle=m) as mg:
        mg.upload(*field(case.field, N))
        mg.profile(True, finest_only=True)
        got = []
        for o in want["outers"]:
            got.append(mg.step_ex(tol))
            assert mg.capped == (o[0] == m)
        n = {k: mg.profile_get(k, 0)[0] for k in (_lib.K_RHS, _lib.K_GS, _lib.K_XSMOOTH)}
        mg.profile(False)
        assert [g[0] for g in got] == [o[0] for o in want["outers"]]
        norms_close([g[1] for g in got], [o[1] for o in want["outers"]], "the steps' r0")
        norms_close([g[2] for g in got], [o[2][-1] for o in want["outers"]], "the steps' last norms")
        bits_equal(mg.download(), want["u"], N, "u after %d capped steps" % steps)
    return n


def test_steps_under_the_cap(oracle_mod, knobs):
    """Three stiff steps at N = 4096 under max_cycle 2 (c* = 6): every step ends
    capped and the next one forms its right-hand side from the unconverged u;
    with the rhs + norm + first pre-smoothing as one pass (step_fuse 1) and as
    two (0): one rhs pass per step in both, one finest-level smoothing pass per
    step fewer in the fused schedule."""
    case, steps, m = E.CAP_STEPS
    want = steps_want(oracle_mod, case, steps, m)
    assert [o[0] for o in want["outers"]] == [m] * steps
    assert all(o[2][-1] / o[1] > case.tol for o in want["outers"])
    n = {}
    for step_fuse in (1, 0):
        knobs(step_fuse=step_fuse)
        n[step_fuse] = steps_case(oracle_mod, case, steps, m)
        assert n[step_fuse][_lib.K_XSMOOTH] > 0
    assert n[1][_lib.K_RHS] == n[0][_lib.K_RHS] == steps, n
    assert n[0][_lib.K_GS] - n[1][_lib.K_GS] == steps, n


@pytest.mark.slow
@pytest.mark.parametrize("m,k_rhs", [(1, 2), (2, 1)])
def test_steps_N8192_step_cross_under_the_cap(oracle_mod, knobs, m, k_rhs):
    """N = 8192, L = 6, easy, bitwise, c* = 2 per step, step_cross 1 (the K_RHS
    counts: see the module docstring)."""
    knobs(step_cross=1)
    case = E.CAP_STEPS_SLOW
    want = steps_want(oracle_mod, case, 2, m)
    assert [o[0] for o in want["outers"]] == [m, m]
    assert [o[2][-1] / o[1] <= case.tol for o in want["outers"]] == [m == 2] * 2
    n = steps_case(oracle_mod, case, 2, m)
    assert n[_lib.K_RHS] == k_rhs, n
    assert n[_lib.K_XSMOOTH] > 0, n


def test_timestepper_under_the_cap(oracle_mod):
    """mgx_timestepper_ex keeps stepping after a capped step, as the
    reference's loop does: MGX_OK, max_cycle cycles per step, uT bitwise."""
    case, steps, m = E.CAP_TIMESTEPPER
    want = steps_want(oracle_mod, case, steps, m)
    assert [o[0] for o in want["outers"]] == [m] * steps
    N = case.N
    dt, nu = F.params(case.params, N)
    u0, v1, v2 = field(case.field, N)
    uT = np.empty_like(u0)
    cyc = pkg.timestepper(uT, u0, v1, v2, nu, case.L, N, dt, (steps + 0.5) * dt, 1.0 / N,
                          case.tol, nsmooth=3, tower_mode=case.tower, fp_mode=case.fp,
                          max_cycle=m)
    assert cyc == [m] * steps
    bits_equal(uT, want["u"], N, "uT of the capped timestepper")


# ---------------------------------------------------------------- C. the coarsest solve

COARSE = [(f, fp, lim) for f in E.COARSE_FORMS for fp in f.fps for lim in E.limits(f)]
KINDS = (_lib.K_GS, _lib.K_COARSE)


def coarse_want(O, form, fp, tol, maxit):
    def make():
        return closing(E.coarse_run(O, form, fp, *field(E.COARSE_FIELD, form.N), tol, maxit),
                       E.coarse_sequence, form.cycles)
    return cached(O, ("coarse", form.N, form.L, form.shape, form.cycles, fp, tol, maxit), fp, make)


@pytest.mark.parametrize("form,fp,lim", COARSE, ids=[
    "%s-%s-tol%g-maxit%d" % (f.name, "fma" if fp else "bitwise", l[0], l[1]) for f, fp, l in COARSE])
def test_coarse_limits(oracle_mod, knobs, form, fp, lim):
    tol, maxit, _ = lim
    want = coarse_want(oracle_mod, form, fp, tol, maxit)
    assert E.coarse_margin(want["coarse_norms"], tol) >= F.MARGIN
    graph = form.keys.get("graph_level", 0)
    knobs(graph_level=0)
    knobs(**form.keys)
    N, L, lc = form.N, form.L, form.L - 1
    dt, nu = E.coarse_params(form)
    g0 = _lib.get_tuning("graph_captures"), _lib.get_tuning("graph_replays")
    with Multigrid(N, L, dt, nu, shape=form.shape, fp_mode=fp, coarse_tol=tol,
                   coarse_maxit=maxit, local_parts=form.parts) as mg:
        mg.upload(*field(E.COARSE_FIELD, N))
        mg.rhs()
        profiled = not graph and not form.parts   # (per-launch profiling turns the replay off)
        if profiled:
            mg.profile(True)
        norms, its = [], []
        for _ in range(form.cycles):
            norms.append(mg.run_cycles(1))
            its.append(mg.coarse_iterations())
        if profiled:
            n = {k: mg.profile_get(k, lc)[0] for k in KINDS}
            n_all = mg.profile_get(_lib.K_COARSE, -1)[0]
            mg.profile(False)
        assert its == want["its"], (its, want["its"], want["visits"])
        bits_equal(mg.download(), want["u"], N, "u after the cycles")
        norms_close(norms, want["norms"], "run_cycles norms")
        info = mg.dist_info() if form.parts else None
    entries = form.cycles * form.shape ** lc
    if form.name in ("lds_fused", "w_cycle_fused"):
        assert n_all == 0, n_all              # solved inside the tile pass above
    elif form.name == "host_loop":
        assert n_all == 0 and n[_lib.K_GS] == want["its"][-1], (n, want["its"])
    elif form.name == "replicated":
        assert info[0] == 2 and 1 <= info[2] <= lc, info   # level 0 in row blocks, lc on every part
    elif form.name == "graph":
        assert _lib.get_tuning("graph_captures") > g0[0]
        assert _lib.get_tuning("graph_replays") > g0[1]    # (cycles 3 and 4: exits.COARSE_FORMS)
    else:
        assert n[_lib.K_COARSE] == n_all == entries and n[_lib.K_GS] == 0, (n, n_all)


# ---------------------------------------------------------------- D. the division's range

SCALES = [-900, 400]


def levels_want(O, N, fp, e):
    def make():
        u0, v1, v2 = field("generic", N)
        dt, nu = F.params("easy", N)
        run = F.CheckerRun(O, np.ldexp(u0, e), v1, v2, N, 3, dt, nu, 0, 3, 1, fp)
        return closing(run, G.seq_levels)
    return cached(O, ("levels", N, fp, e), fp, make)


def levels_run(mg, N, u0, v1, v2):
    """seq_levels on the solver -> dict of what the checker's returns."""
    out = {}
    mg.upload(u0, v1, v2)
    mg.rhs()
    out["rhs"] = mg.download_level(0, "rhs")
    mg.profile(True)
    mg.gs(0, 3)
    assert mg.profile_get(_lib.K_GS, 0)[0] >= 1
    mg.profile(False)
    out["u_gs"] = mg.download()
    out["norm"] = mg.residual_norm(0)
    mg.restrict(0)
    out["rhs1"] = mg.download_level(1, "rhs")
    mg.gs(1, 1)
    out["u1"] = mg.download_level(1, "u")
    mg.prolong_add(0)
    out["u_pr"] = mg.download()
    return out


@pytest.mark.parametrize("fp", [E.BIT, E.FMA], ids=["bitwise", "fma"])
@pytest.mark.parametrize("e", SCALES, ids=["2^-900", "2^+400"])
@pytest.mark.parametrize("N", [128, 512])
def test_level_passes_scaled(oracle_mod, N, e, fp, tile_mode):
    """Smoother 0, fuse 3, as tiles and as the forced march: far from 1 but
    inside the division's domain everything is bitwise."""
    want = levels_want(oracle_mod, N, fp, e)
    u0, v1, v2 = field("generic", N)
    dt, nu = F.params("easy", N)
    n1 = N // 2
    with Multigrid(N, 3, dt, nu, smoother=0, fuse=3, fp_mode=fp) as mg:
        got = levels_run(mg, N, np.ldexp(u0, e), v1, v2)
    assert np.array_equal(G.interior(got["rhs"], N), G.interior(want["rhs"], N))
    bits_equal(got["u_gs"], want["u_gs"], N, "u after gs(0, 3)")
    assert np.array_equal(G.interior(got["rhs1"], n1), G.interior(want["rhs1"], n1))
    bits_equal(got["u1"], want["u1"], n1, "u[1] after gs(1, 1)")
    bits_equal(got["u_pr"], want["u_pr"], N, "u after prolong_add(0)")
    assert np.all(np.isfinite(want["u_pr"])) and want["u_pr"].any()
    if e < 0:
        assert want["norm"] == 0.0 and want["norm"].exact == 0.0   # the squares underflow
        assert got["norm"] == 0.0
    else:
        norms_close([got["norm"]], [want["norm"]], "residual_norm(0)")


tile_mode = G.tile_mode


def ulps(a, b):
    """|a - b| in units in the last place of doubles of one sign (both finite)."""
    ia, ib = a.view(np.int64), b.view(np.int64)
    mag = lambda i: np.where(i < 0, np.int64(-2 ** 63) - i, i)     # (monotonic in the value)
    return np.abs(mag(ia) - mag(ib))


@pytest.mark.parametrize("N", [128, 512])
def test_level_passes_below_the_division_threshold(oracle_mod, N, tile_mode):
    """u0 scaled by 2^-1000, bitwise mode: the numerators of gs(0, 3) lie below
    the threshold, where the fused pass's quotient may be the neighbour of the
    correctly rounded one.  Every entry within one ulp of the checker's; the
    mismatching share is printed and recorded in the module docstring, not
    bounded.  Smoother 1 divides: bitwise."""
    e = -1000
    want = levels_want(oracle_mod, N, E.BIT, e)
    u0, v1, v2 = field("generic", N)
    dt, nu = F.params("easy", N)
    with Multigrid(N, 3, dt, nu, smoother=1, fuse=3) as mg:
        exact = levels_run(mg, N, np.ldexp(u0, e), v1, v2)
    for k in ("u_gs", "u1", "u_pr"):
        bits_equal(exact[k], want[k], N if k != "u1" else N // 2, k + " (smoother 1)")
    with Multigrid(N, 3, dt, nu, smoother=0, fuse=3) as mg:
        got = levels_run(mg, N, np.ldexp(u0, e), v1, v2)
    assert np.array_equal(G.interior(got["rhs"], N), G.interior(want["rhs"], N))
    share = {}
    for k in ("u_gs", "u1", "u_pr"):
        d = ulps(got[k], want[k])
        share[k] = float(np.count_nonzero(d)) / d.size
        print("N=%d %s: %d of %d entries differ, max %d ulp" % (N, k, np.count_nonzero(d), d.size,
                                                                 d.max()))
        assert d.max() <= 1, (k, int(d.max()), share[k])
    assert got["norm"] == 0.0 == want["norm"]


# ---------------------------------------------------------------- a NaN

def test_one_nan(oracle_mod):
    """One NaN in the interior of u0 at N = 256, L = 3: mg_outer runs no cycle
    and is not capped (`res / res0 > tol` is false for a NaN, as in the
    checker's loop); two cycles spread it exactly as the checker's do, the
    finite entries bitwise; a coarsest solve with a NaN norm ends after one
    sweep."""
    O = oracle_mod
    u0, v1, v2 = E.nan_field()
    want = cached(O, "nan", E.BIT, lambda: closing(E.nan_run(O, u0, v1, v2), E.nan_sequence))
    assert want["outer"][0] == 0 and want["its"] == 2
    N = E.NAN_N
    dt, nu = F.params(E.NAN_PARAMS, N)
    with Multigrid(N, E.NAN_L, dt, nu) as mg:
        mg.upload(u0, v1, v2)
        mg.rhs()
        cyc, r0, r, capped = mg.mg_outer(1e-6)
        assert (cyc, capped) == (0, False) and np.isnan(r0) and np.isnan(r)
        assert np.isnan(mg.run_cycles(2))
        assert mg.coarse_iterations() == want["its"]
        got = mg.download()
    nan = np.isnan(want["u"])
    assert np.array_equal(np.isnan(got), nan) and 0 < nan.sum() < nan.size
    assert np.array_equal(got[~nan].view(np.uint64), want["u"][~nan].view(np.uint64))

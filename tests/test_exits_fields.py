"""CPU: the conditions tests/test_gpu_exits.py rests on, on the checker alone
(tests/exits.py holds the cases, the mirror of mg_inner and the figures).

  * exits.mg_inner equals or_mg_inner bit for bit at the default limits: u, every
    level's u and rhs as uint64, and the returned sweep count -- V and W, both
    towers, both fp modes, nsmooth 0 .. 4, N = 64 and 256, two cycles each.
  * Every coarse-limit case keeps fields.MARGIN between coarse_tol and every
    coarsest norm of every visit, stays finite, and stops the way its name says.
    "cap": the first visit is ended by the sweep cap with its norm still above
    coarse_tol, and no visit runs more sweeps than the cap.  "tol": every visit
    ends below coarse_tol before the cap of 50, the first one after 2 .. 40
    sweeps and none after more than 40.  (Not "every visit after 2 .. 40": the
    second visit of a W-cycle's pair starts from the first one's solution and
    ends after one sweep -- which is what makes the per-visit counts differ.)
  * Every cycle-cap case keeps fields.MARGIN between tol and every r_k / r_0 of
    both mg_outer calls and of every step, the growth case grows and stays
    finite, and the counts are the ones the cases' names promise.
The N = 8192 steps of tests/test_gpu_exits.py are checked there, from the
checker run that file makes anyway.  This file takes 100 s on 8 threads, 80 of
them the six N = 4096 runs.
"""
import numpy as np
import pytest

import exits as E
import fields as F


@pytest.fixture
def checker(oracle_mod):
    O = oracle_mod
    O.set_threads(16)
    yield O
    O.set_fp_mode(0)
    O.set_threads(1)


# ---------------------------------------------------------------- the mirror

@pytest.mark.parametrize("shape", [E.V, E.W], ids=["V", "W"])
@pytest.mark.parametrize("N,L", [(64, 1), (64, 3), (256, 2), (256, 4)])
def test_mirror_equals_or_mg_inner(checker, N, L, shape):
    O = checker
    u0, v1, v2 = F.make("generic", N)
    dt, nu = F.params("visc16", N)
    for tower in (E.REF, E.COR):
        for fp in (E.BIT, E.FMA):
            O.set_fp_mode(fp)
            for nsmooth in range(5):
                what = (tower, fp, nsmooth)
                a = F.CheckerRun(O, u0, v1, v2, N, L, dt, nu, tower, nsmooth, shape, fp)
                b = E.Run(O, u0, v1, v2, N, L, dt, nu, tower, nsmooth, shape, fp)
                try:
                    a.rhs()
                    b.rhs()
                    for _ in range(2):
                        a.mg_inner()
                        b.mg_inner()
                        assert a.coarse_its == b.coarse_its == sum(b.visits), what
                        assert np.array_equal(a.u.view(np.uint64), b.u.view(np.uint64)), what
                        for l in range(L):
                            for w in ("u", "rhs"):
                                assert np.array_equal(a.t.level(w, l).view(np.uint64),
                                                      b.t.level(w, l).view(np.uint64)), (what, l, w)
                    assert len(b.visits) == len(b.coarse_norms) == 2 * shape ** L, what
                    assert [len(x) for x in b.coarse_norms] == b.visits, what
                finally:
                    a.close()
                    b.close()


# ---------------------------------------------------------------- the coarsest solve

COARSE = [(f, fp, lim) for f in E.COARSE_FORMS for fp in f.fps for lim in E.limits(f)]


def coarse_id(f, fp, lim):
    return "%s-%s-tol%g-maxit%d" % (f.name, "fma" if fp else "bitwise", lim[0], lim[1])


def test_the_forms_reach_what_they_name():
    n = {f.name: f.N >> (f.L - 1) for f in E.COARSE_FORMS}
    assert n["lds_fused"] == n["lds"] == n["l2_n64"] == n["w_cycle"] == n["replicated"] == 64
    assert n["l2_n256"] == 256 and n["host_loop"] == 512 and n["finest"] == 64
    assert all(set(f.fps) == {E.BIT, E.FMA} for f in E.COARSE_FORMS if f.name[:2] in ("ld", "l2"))
    for f in E.COARSE_FORMS:
        lims = E.limits(f)
        assert [l[1] for l in lims] == [1, 2, 7, 50, 50, 5]
        assert [l[0] for l in lims[:3]] == [1e-5] * 3 and lims[5][0] == 0.0
        assert lims[3][0] > 1e3 * lims[4][0] > 0 and 1e-5 not in (lims[3][0], lims[4][0])
        assert all(l[1] <= 50 for l in lims)


@pytest.mark.parametrize("form,fp,lim", COARSE, ids=[coarse_id(*c) for c in COARSE])
def test_coarse_limits_keep_the_margin_and_stop_as_named(checker, form, fp, lim):
    O = checker
    tol, maxit, how = lim
    O.set_fp_mode(fp)
    run = E.coarse_run(O, form, fp, *F.make(E.COARSE_FIELD, form.N), tol, maxit)
    try:
        want = E.coarse_sequence(run, form.cycles)
    finally:
        run.close()
    print(want["visits"], "%.3g" % E.coarse_margin(want["coarse_norms"], tol), want["norms"])
    assert np.all(np.isfinite(want["u"])) and np.all(np.isfinite(want["norms"]))
    assert E.coarse_margin(want["coarse_norms"], tol) >= F.MARGIN
    counts = [v for cyc in want["visits"] for v in cyc]
    assert len(counts) == form.cycles * form.shape ** form.L and want["its"][-1] == sum(counts)
    first = want["coarse_norms"][0]
    if how == "cap":
        assert counts[0] == maxit and first[-1] > tol
        assert max(counts) <= maxit
    else:
        assert all(len(v) < maxit and v[-1] <= tol for v in want["coarse_norms"])
        assert 2 <= counts[0] <= 40 and max(counts) <= 40


def test_w_cycle_visits_differ(checker):
    """A launch that applied the first visit's count to both visits of a pair
    would be wrong in every tolerance case and right in every cap case but the
    first: the counts of a pair differ."""
    O = checker
    O.set_fp_mode(E.FMA)
    form = next(f for f in E.COARSE_FORMS if f.name == "w_cycle")
    for tol, maxit, how in E.limits(form):
        run = E.coarse_run(O, form, E.FMA, *F.make(E.COARSE_FIELD, form.N), tol, maxit)
        try:
            want = E.coarse_sequence(run)
        finally:
            run.close()
        pairs = [(c[i], c[i + 1]) for c in want["visits"] for i in range(0, len(c), 2)]
        if how == "tol":
            assert all(a >= b == 1 for a, b in pairs), pairs
            assert all(a > b for a, b in pairs[:4]), pairs      # (every pair of the first cycle)
        else:
            assert all(a == b == maxit for a, b in pairs), pairs


# ---------------------------------------------------------------- the cycle cap

def outers_ok(outers, tol):
    for r0, norms in outers:
        assert np.isfinite(r0) and np.all(np.isfinite(norms)), (r0, norms)
        assert F.margin(r0, norms, tol) >= F.MARGIN, (r0, norms)


def cap_want(O, case, caps):
    O.set_fp_mode(case.fp)
    run = E.cap_run(O, case, *F.make(case.field, case.N))
    try:
        return E.cap_sequence(run, caps, case.tol)
    finally:
        run.close()


def cap_outers(want):
    return [(want["r0"], want["norms"])] + [c["second"][1:] for c in want["caps"].values()]


CAP_4096 = [(E.CAP_MAIN, E.CAP_MAIN_CAPS, 6), (E.CAP_W, E.CAP_W_CAPS, 3)] + \
    [(c, caps, 6) for c, caps in E.CAP_OTHER]


@pytest.mark.parametrize("case,caps,cstar", CAP_4096, ids=[E.cap_id(c[0]) for c in CAP_4096])
def test_cap_cases_at_N4096(checker, case, caps, cstar):
    want = cap_want(checker, case, caps)
    outers_ok(cap_outers(want), case.tol)
    r0, norms = want["r0"], want["norms"]
    assert cstar in caps                       # "converged on the last allowed cycle"
    assert [r / r0 <= case.tol for r in norms] == [False] * (cstar - 1) + [True]
    for m, c in want["caps"].items():
        assert c["first"] == min(m, cstar)
        cyc, r0s, ns = c["second"]
        assert cyc == m and ns[-1] / r0s > case.tol     # the second call ends capped too
        assert np.all(np.isfinite(c["u2"]))


@pytest.mark.parametrize("case,caps", E.CAP_SMALL, ids=[E.cap_id(c) for c, _ in E.CAP_SMALL])
def test_cap_cases_without_the_cross_pass_contract(checker, case, caps):
    want = cap_want(checker, case, caps)
    outers_ok(cap_outers(want), case.tol)
    r0, norms = want["r0"], want["norms"]
    assert len(norms) == 2 and norms[1] < norms[0] < r0 and norms[1] / r0 > case.tol
    assert want["caps"][2]["second"][0] == 2


def test_growth_case_grows_and_stays_finite(checker):
    case = E.CAP_GROWTH
    want = cap_want(checker, case, E.CAP_GROWTH_CAPS)
    outers_ok(cap_outers(want), case.tol)
    for r0, norms in cap_outers(want):
        seq = [r0] + list(norms)
        assert len(norms) == 4 and all(b > 2 * a for a, b in zip(seq, seq[1:])), seq
    assert np.all(np.isfinite(want["caps"][4]["u2"]))


def test_growth_case_with_the_cross_pass_grows_and_stays_finite(checker):
    case = E.CAP_GROWTH_CROSS
    want = cap_want(checker, case, E.CAP_GROWTH_CAPS)
    outers_ok(cap_outers(want), case.tol)
    r0, norms = want["r0"], want["norms"]
    assert len(norms) == 4 and norms[1] < norms[2] < norms[3] < r0
    cyc, r4, more = want["caps"][4]["second"]
    seq = [r4] + list(more)
    assert cyc == 4 and all(b > 1.3 * a for a, b in zip(seq, seq[1:])), seq
    assert np.all(np.isfinite(want["caps"][4]["u2"]))


def test_timestepper_case_is_capped_every_step(checker):
    case, steps, cap = E.CAP_TIMESTEPPER
    O = checker
    O.set_fp_mode(case.fp)
    for m in (50, cap):
        run = E.cap_run(O, case, *F.make(case.field, case.N))
        try:
            want = E.cap_steps_sequence(run, steps, m, case.tol)
        finally:
            run.close()
        outers_ok([o[1:] for o in want["outers"]], case.tol)
        if m == 50:
            assert all(cap < o[0] < 50 for o in want["outers"])      # c* > cap
        else:
            assert [o[0] for o in want["outers"]] == [cap] * steps
        assert np.all(np.isfinite(want["u"]))


def test_steps_case_is_capped_every_step(checker):
    case, steps, cap = E.CAP_STEPS
    O = checker
    O.set_fp_mode(case.fp)
    run = E.cap_run(O, case, *F.make(case.field, case.N))
    try:
        want = E.cap_steps_sequence(run, steps, cap, case.tol)
    finally:
        run.close()
    outers_ok([o[1:] for o in want["outers"]], case.tol)
    assert [o[0] for o in want["outers"]] == [cap] * steps
    assert all(o[2][-1] / o[1] > case.tol for o in want["outers"])


# ---------------------------------------------------------------- a NaN

def test_nan_ends_every_loop_at_once(checker):
    """The checker's loops on a field with one NaN: mg_outer's `res / res0 >
    tol` is false at once (0 cycles), a coarsest solve ends after one sweep,
    and two cycles spread the NaN without touching the ring."""
    O = checker
    O.set_fp_mode(E.BIT)
    u0, v1, v2 = E.nan_field()
    run = E.nan_run(O, u0, v1, v2)
    try:
        want = E.nan_sequence(run)
    finally:
        run.close()
    assert want["outer"][0] == 0 and np.isnan(want["outer"][1])
    assert want["visits"] == [1, 1] and want["its"] == 2
    nan = np.isnan(want["u"]).reshape(E.NAN_N + 1, E.NAN_N + 1)
    assert nan[1:-1, 1:-1].any() and not nan[0].any() and not nan[:, 0].any()
    assert not nan[-1].any() and not nan[:, -1].any()
    assert not np.isinf(want["u"]).any()

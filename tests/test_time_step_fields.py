"""CPU: the conditions tests/test_gpu_time_step.py relies on, on the checker
alone (tests/tsteps.py, tests/fields.py).

A theta-scheme step means compute_rhs with k = kB, the source term, a pending
ring, then mg_outer with k = kA (tsteps.checker_steps).  Every case the GPU
tests run against the checker (tsteps.CASES) must stay finite, converge under
the cycle cap and keep every r_k / r_0 at least fields.MARGIN (1 %) away from
the tolerance, so that a cycle count never hinges on a summation order.  This
is a condition, not a measurement.  Measured with the checker (tol 1e-9, seed
1; SEQ_EASY unless stated; cycles per step, smallest margin over the steps):
  N=128  L=3 easy generic            : 2,2,2,2,12,2  0.58
  N=128  L=3 easy generic0           : 2,2,2,2,12,2  0.65
  N=128  L=3 easy generic, separable source + rings (None,0,None,1,2,None)
                                     : 2,2,2,2,12,2  0.39
  N=256  L=4 easy generic (fma)      : 2,2,2,2,10,2  0.25
  N=1024 L=6 easy generic            : 2,2,2,2,4,2   0.15
  N=1024 L=6 easy generic, correct tower (fma): 2,2,2,2,4,2  0.14
  N=4096 L=6 easy generic (fma)      : 2,2,2,2,4,2   0.85
  N=4096 L=7 easy generic            : 2,2,2,2,4,2   0.85
  N=4096 L=7 easy rank1 (fma)        : 2,2,2,2,4,2   0.88
  N=4096 L=7 stiff generic, SEQ_STIFF: 6,6,4,6,7     0.23
Avoided: rank1 with the source at N=1024 (margin 0.001), "stiff" at N=128 (the
checker diverges, tests/fields.py), any N=8192 checker run (a minute a run).
"""
import numpy as np
import pytest

import fields as F
import rings as R
import tsteps as T


@pytest.fixture
def checker(oracle_mod):
    O = oracle_mod
    O.set_threads(16)
    yield O
    O.set_fp_mode(0)
    O.set_threads(1)


def test_k_pair_is_exact_at_crank_nicolson():
    for N in (8, 128, 4096, 8192):
        for pname in F.PARAMS:
            dt0 = F.params(pname, N)[0]
            for m in (1, .5, 2, 3, .7, .25):
                dt = np.float64(m) * np.float64(dt0)
                kA, kB = T.k_pair(dt, .5)
                assert kA == kB == dt
    kA, kB = T.k_pair(.01, 1)
    assert (kA, kB) == (.02, 0.0)
    kA, kB = T.k_pair(.01, .75)
    assert kA == np.float64(1.5) * np.float64(.01) and kB == np.float64(.5) * np.float64(.01)
    # the sequences start with a step that needs no call
    for seq in (T.SEQ_EASY, T.SEQ_STIFF, T.SEQ_FUSE):
        assert seq[0] == (1, .5)


@pytest.mark.parametrize("fp", [0, 1], ids=["bitwise", "fma"])
def test_the_loop_at_crank_nicolson_is_checker_step(checker, fp):
    """tsteps.checker_steps with theta = .5, m = 1 is CheckerRun.step, bit for
    bit: u, every norm, the cycle counts."""
    O = checker
    O.set_fp_mode(fp)
    N, L = 128, 3
    dt, nu = F.params("easy", N)
    a = F.CheckerRun(O, *F.make("generic", N), N, L, dt, nu, 0, fp=fp)
    b = F.CheckerRun(O, *F.make("generic", N), N, L, dt, nu, 0, fp=fp)
    try:
        got = T.checker_steps(a, dt, ((1, .5),) * 3)
        for k in range(3):
            cyc, r0, norms = b.step(T.TOL)
            assert (cyc, float(r0), [float(x) for x in norms]) == (
                got[k][0], float(got[k][1]), [float(x) for x in got[k][2]]), k
            assert r0.exact == got[k][1].exact
            assert np.array_equal(b.u.view(np.uint64), got[k][3].view(np.uint64)), k
        assert a.dt == dt
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize(T.CASE_ARGS, T.CASE_PARAMS, ids=T.CASE_IDS)
def test_no_cycle_norm_sits_at_the_tolerance(checker, N, L, pname, name, tower, fp, seq, extra,
                                             nsmooth, fuse, shape):
    O = checker
    O.set_fp_mode(fp)
    dt, nu = F.params(pname, N)
    run = F.CheckerRun(O, *F.make(name, N), N, L, dt, nu, tower, nsmooth, shape, fp)
    try:
        steps = T.checker_steps(run, dt, seq, T.TOL, T.source_field(N)[2] if extra else None,
                                T.RINGS if extra else None, keep_u=False)
        finite = bool(np.all(np.isfinite(run.u)))
    finally:
        run.close()
    print([(c, F.margin(r0, norms, T.TOL)) for c, r0, norms, _ in steps])
    assert finite
    for k, (cyc, r0, norms, _) in enumerate(steps):
        assert np.isfinite(r0) and np.all(np.isfinite(norms)), (k, r0, norms)
        assert cyc < 50 and norms[-1] / r0 <= T.TOL, (k, cyc, r0, norms)
        assert F.margin(r0, norms, T.TOL) >= F.MARGIN, (k, r0, norms)

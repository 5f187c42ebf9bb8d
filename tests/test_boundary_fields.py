"""CPU: the conditions tests/test_gpu_boundary.py relies on, on the checker
alone (tests/rings.py, tests/fields.py).

A step with a ring pending means rhs() with the old ring, the new ring, then
mg_outer with its own initial norm (rings.checker_steps).  Every case the GPU
tests run through mg_outer (rings.CASES) must converge with every r_k / r_0 at
least fields.MARGIN (1 %) away from the tolerance, so that a cycle count never
hinges on a summation order.  This is a condition, not a measurement.  Measured
with the checker (tol 1e-9; the same counts and margins in both fp modes):
  N=128  L=3 easy : 2, 2, 2 cycles per step, smallest margin 0.90
  N=1024 L=6 easy : 2, 2, 2, margin 0.14
  N=4096 L=7 stiff: 6, 7, 7, margin 0.22
  N=4096 L=7 easy : 2, 2, 2, margin 1.0
  N=4096 L=6 easy (the partitioned contexts' tower): 2, 2, 2, margin 1.0
  N=1024 L=6 easy, correct tower (upload_rows): 2, 2, 2, margin 0.13
  N=128  L=3 easy with the separable source: 2, 2, 2, margin 0.87
  N=8192 L=8 easy, fma, two plain steps, a ring step, a plain step: 2 cycles
    each, margins 0.78 0.82 0.75 0.48
The stiff time step is not used at N=128 or N=1024: there the checker itself
diverges (tests/test_fields.py).  The cases run at the GPU tests' own sizes;
the N=8192 one is the slow one (four steps on 6.7e7 points, 40 s with 16
threads), the N=4096 stiff ones take 12 s and 22 s.
"""
import numpy as np
import pytest

import fields as F
import rings as R


@pytest.fixture
def checker(oracle_mod):
    O = oracle_mod
    O.set_threads(16)
    yield O
    O.set_fp_mode(0)
    O.set_threads(1)


@pytest.mark.parametrize("N", [1, 2, 7, 128])
def test_put_then_get_is_the_ring_with_the_corner_rule(N):
    rng = np.random.default_rng(N)
    u = rng.standard_normal((N + 1) ** 2)
    before = u.copy()
    g = R.ring(N, 3)
    assert g.shape == (4, N + 1) and g.dtype == np.float64
    R.put(u, N, g)
    U, B = u.reshape(N + 1, N + 1), before.reshape(N + 1, N + 1)
    assert np.array_equal(U[1:N, 1:N], B[1:N, 1:N])            # the interior is untouched
    got = R.get(u, N)
    assert np.array_equal(got, R.corner_rule(g, N))
    assert np.array_equal(got[0], g[0]) and np.array_equal(got[1], g[1])   # the rows win
    assert np.array_equal(got[2, 1:N], g[2, 1:N]) and np.array_equal(got[3, 1:N], g[3, 1:N])
    assert (got[2, 0], got[2, N], got[3, 0], got[3, N]) == (g[0, 0], g[1, 0], g[0, N], g[1, N])


def test_rings_differ_from_step_to_step_and_are_reproducible():
    N = 64
    gs = [R.ring(N, k) for k in range(3)]
    for k in range(3):
        assert np.array_equal(gs[k], R.ring(N, k))
        assert np.all(gs[k] != 0) and np.ptp(gs[k]) > 0.5
        for j in range(k):
            assert np.abs(gs[k] - gs[j]).max() > 0.1


CASE_IDS = ["N%d-L%d-%s-%s-t%d-%s%s%s" % (N, L, p, f, tw, "bitwise" if fp == 0 else "fma",
                                          "" if seq == R.RING3 else "-mixed",
                                          "-source" if src else "")
            for N, L, p, f, tw, fps, seq, src in R.CASES for fp in fps]
CASE_PARAMS = [(N, L, p, f, tw, fp, seq, src)
               for N, L, p, f, tw, fps, seq, src in R.CASES for fp in fps]


@pytest.mark.parametrize("N,L,pname,field,tower,fp,seq,src", CASE_PARAMS, ids=CASE_IDS)
def test_no_cycle_norm_sits_at_the_tolerance(checker, N, L, pname, field, tower, fp, seq, src):
    O = checker
    O.set_fp_mode(fp)
    dt, nu = F.params(pname, N)
    source = None
    if src:
        a, b = R.source_factors(N)
        source = (a[:, None] * b[None, :]).ravel()
    run = F.CheckerRun(O, *F.make(field, N), N, L, dt, nu, tower, fp=fp)
    try:
        steps = R.checker_steps(run, seq, R.TOL, source, keep_u=False)
    finally:
        run.close()
    print([(c, F.margin(r0, norms, R.TOL)) for c, r0, norms, _ in steps])
    for k, (cyc, r0, norms, _) in enumerate(steps):
        assert cyc < 50 and norms[-1] / r0 <= R.TOL, (k, cyc, r0, norms)
        assert F.margin(r0, norms, R.TOL) >= F.MARGIN, (k, r0, norms)

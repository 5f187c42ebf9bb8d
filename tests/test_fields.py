"""CPU: the generated test fields (tests/fields.py) have the properties the GPU
tests of tests/test_gpu_generic_fields.py rely on, checked where no GPU is
needed -- the host factorisation, the CPU checker's towers and the checker's
own convergence history.

Convergence conditions.  Measured with the checker (seed 1, reference tower,
nsmooth 3, V-cycles, tol 1e-9), r_k / r_0 per cycle:
  easy,  N=512  L=3: 2 cycles: 2.0e-9, 4.2e-15 (the rounding floor)
  stiff, N=2048 L=3: 7 cycles: 6.2e-3 2.1e-4 1.0e-5 5.9e-7 3.6e-8 2.2e-9 1.4e-10
  stiff, N=4096 L=5: 6 cycles: 3.8e-3 1.3e-4 5.7e-6 2.7e-7 1.3e-8 6.5e-10
                     (r_0 = 1535; steps 2, 3: 6 cycles each, last 7.7e-10, 8.9e-10)
The stiff parameters (dt = 1/N) DIVERGE in the checker at N <= 1024 (N=1024:
r_k / r_0 = 0.37, 1.0, 4.1, 19, ...; N=512: 8.4, 519, ...): with dt|v|/h fixed
at ~3.3 the diffusion number dt|nu|/h^2 = 4e-4 N is what keeps the sweeps
contracting, and it is too small there.  So the stiff cases are checked at
N=2048, the smallest power of two at which they converge, and the easy ones at
N=512; the GPU tests assert the same condition at their own sizes.
"""
import numpy as np
import pytest

import fields as F
from fields import factor


@pytest.fixture
def checker(oracle_mod):
    O = oracle_mod
    O.set_threads(8)
    yield O
    O.set_fp_mode(0)
    O.set_threads(1)


def ring(a, N):
    a = a.reshape(N + 1, N + 1)
    return np.concatenate([a[0], a[N], a[:, 0], a[:, N]])


@pytest.mark.parametrize("N", [16, 128, 512])
def test_generic_has_the_stated_properties(N):
    u, v1, v2 = F.generic(N, F.SEED)
    for a in (u, v1, v2):
        assert a.dtype == np.float64 and a.shape == ((N + 1) ** 2,) and a.flags["C_CONTIGUOUS"]
    r = ring(u, N)
    assert np.all(r != 0) and np.ptp(r) > 0.5          # non-zero, non-constant Dirichlet data
    assert np.median(np.abs(u)) > 0.05                 # O(1) everywhere, no 1e-40 plateau
    for v in (v1, v2):
        assert np.abs(v).max() <= 3.5
        assert v.min() < -0.5 and v.max() > 0.5        # sign changes
        assert np.all(ring(v, N) != 0)
        V = v.reshape(N + 1, N + 1)
        assert np.linalg.matrix_rank(V[:12, :12]) == 12   # noise: nowhere near separable
    V1, V2 = v1.reshape(N + 1, N + 1), v2.reshape(N + 1, N + 1)
    for W in (V2, V2.T, -V2, -V2.T):                   # no symmetry between v1 and v2
        assert np.abs(V1 - W).max() > 1.0
    u0, w1, w2 = F.generic(N, F.SEED, boundary=False)
    assert not ring(u0, N).any()
    assert np.array_equal(w1, v1) and np.array_equal(w2, v2)
    U, U0 = u.reshape(N + 1, N + 1), u0.reshape(N + 1, N + 1)
    assert np.array_equal(U[1:N, 1:N], U0[1:N, 1:N])
    # a pure function of (N, seed)
    assert all(np.array_equal(a, b) for a, b in zip(F.generic(N, F.SEED), (u, v1, v2)))
    assert not np.array_equal(F.generic(N, F.SEED + 1)[0], u)


@pytest.mark.parametrize("N", [64, 512, 4096])
def test_factorisation_refuses_generic_and_reproduces_rank1(N):
    """mgx_factor_velocity (host only), smin as at upload: "bitwise or refuse"."""
    _, v1, v2 = F.generic(N, F.SEED)
    assert not factor(v1, N, smin=0.5 / N)[0]
    assert not factor(v2, N, smin=0.5 / N)[0]
    for v in F.rank1_flow(N, F.SEED):
        ok, a, b = factor(v, N, smin=0.5 / N)
        assert ok
        assert np.array_equal(np.multiply.outer(a, b).ravel().view(np.uint64), v.view(np.uint64))


@pytest.mark.parametrize("N", [64, 4096])
def test_rank1_factors_have_the_stated_properties(N):
    a1, b1, a2, b2 = F.rank1_factors(N, F.SEED)
    j1, j2 = F.rank1_unit_columns(N)
    assert b1[j1] == 1.0 and b2[j2] == 1.0
    assert j1 not in (0, (N + 1) // 2) and j2 not in (0, (N + 1) // 2)
    x = np.arange(N + 1) / N
    for f in (a1, b1, a2, b2):
        z = f == 0
        assert z.sum() == 3 and np.signbit(f[z]).sum() == 1       # zeros, one of them -0.0
        m = np.abs(f[~z])
        assert m.min() == 1e-3 and m.max() == 1.8
        assert f.min() < -0.5 and f.max() > 0.5
        # not a sinusoid: the best fit of one leaves the noise
        A = np.stack([np.sin(2.3 * np.pi * x), np.cos(2.3 * np.pi * x), x, np.ones_like(x)], 1)
        res = f - A @ np.linalg.lstsq(A, f, rcond=None)[0]
        assert np.std(res) > 0.1
    v1, v2 = F.rank1_flow(N, F.SEED)
    assert np.abs(v1).max() <= 3.5 and np.abs(v2).max() <= 3.5
    V1 = v1.reshape(N + 1, N + 1)
    assert np.array_equal(V1[:, j1].view(np.uint64), a1.view(np.uint64))
    assert np.signbit(V1[a1 == 0]).any() and not np.signbit(V1[a1 == 0]).all()


def test_reference_tower_of_generic_has_zero_rows_and_the_correct_tower_none(checker):
    """The reference's injection quirk leaves 3/4 of level 1's velocity rows
    zero whatever the field (measured at N=4096: 1536 of 2049); the correct
    tower of generic() has none, so the kernels' zero-row shortcut must not
    fire there."""
    O = checker
    N, L = 512, 3
    u0, v1, v2 = F.generic(N, F.SEED)
    for tower, want in ((0, 3 * N // 8), (1, 0)):
        t = O.Tower(u0, v1, v2, N, L, tower)
        try:
            n = N // 2
            for name in ("v1", "v2"):
                V = t.level(name, 1)[: (n + 1) ** 2].reshape(n + 1, n + 1)
                assert int((~V.any(axis=1)).sum()) == want, (tower, name)
        finally:
            t.close()


@pytest.mark.parametrize("fp", [0, 1], ids=["bitwise", "fma"])
def test_checker_run_is_the_checkers_own_loops(checker, fp):
    """fields.CheckerRun (the loops driven from Python, keeping every norm)
    against or_mg_outer and or_timestepper: the same bits and counts."""
    O = checker
    O.set_fp_mode(fp)
    N, L = 128, 3
    dt, nu = F.params("easy", N)
    u0, v1, v2 = F.generic(N, F.SEED)
    t = O.Tower(u0, v1, v2, N, L)
    O.compute_rhs(t.ufine, N, v1, v2, dt, nu, 1.0 / N, rhs=t.rhsfine)
    cyc, r0, r = t.mg_outer(dt, nu, 1e-12)
    run = F.CheckerRun(O, u0, v1, v2, N, L, dt, nu, fp=fp)
    run.rhs()
    c2, r02, norms = run.mg_outer(1e-12)
    assert (c2, r02, norms[-1]) == (cyc, r0, r)
    assert np.array_equal(run.u, t.ufine)
    t.close()
    run.close()
    want, cyc_ref = O.timestepper(u0, v1, v2, nu, L, N, dt, 3.5 * dt, 1.0 / N, tol=F.TOL)
    run = F.CheckerRun(O, u0, v1, v2, N, L, dt, nu, fp=fp)
    assert [run.step(F.TOL)[0] for _ in range(3)] == cyc_ref
    assert np.array_equal(run.u, want)
    run.close()


def test_accurate_norm_is_fsum_and_the_serial_sum_is_within_its_bound(checker):
    """fields.Norm: .exact equals math.fsum of the squared residual to 1e-15;
    the checker's serial sum lies within M eps / 2 of it -- its own error
    bound, which at the GPU tests' sizes is far above the 1e-11 the solver's
    norms are held to."""
    import math
    O = checker
    N, L = 512, 3
    dt, nu = F.params("easy", N)
    run = F.CheckerRun(O, *F.make("generic", N), N, L, dt, nu)
    try:
        run.rhs()
        for take in (lambda: run.norm(reference_form=True), run.cycle, run.cycle):
            r = take()   # (its residual is in run.t.tmp until the next one)
            sq = run.t.tmp.reshape(N + 1, N + 1)[1:N, 1:N] ** 2
            exact = math.sqrt(math.fsum(sq.ravel().tolist()))
            assert abs(r.exact - exact) <= 1e-15 * exact
            assert float(r) == O.compute_norm(run.t.tmp, N)
            assert abs(float(r) - exact) <= 0.5 * sq.size * np.finfo(float).eps * exact
    finally:
        run.close()


@pytest.mark.parametrize("tower", [0, 1], ids=["reference", "correct"])
@pytest.mark.parametrize("field,pname,nsmooth,shape,tol", F.CONVERGENCE_CASES)
def test_no_cycle_norm_sits_at_the_tolerance(checker, field, pname, nsmooth, shape, tol, tower):
    """Three time steps of every case a GPU test runs through mg_outer / step:
    it converges, and every r_k / r_0 is at least 1 % away from tol, so that a
    cycle count cannot hinge on a summation order.  (Sizes: module docstring.)"""
    O = checker
    N = 2048 if pname == "stiff" else 512
    L = 3 if nsmooth == 3 and shape == 1 else 2
    dt, nu = F.params(pname, N)
    run = F.CheckerRun(O, *F.make(field, N), N, L, dt, nu, tower, nsmooth, shape)
    try:
        for step in range(3):
            cyc, r0, norms = run.step(tol)
            assert cyc < 50 and norms[-1] / r0 <= tol, (step, cyc, r0, norms)
            assert F.margin(r0, norms, tol) >= F.MARGIN, (step, r0, norms)
    finally:
        run.close()


def test_stiff_parameters_need_the_large_grids(checker):
    """Why the stiff cases above do not run at N=512: there the checker's
    V-cycle diverges (the norm grows from the first cycle on)."""
    O = checker
    N, L = 512, 3
    dt, nu = F.params("stiff", N)
    run = F.CheckerRun(O, *F.make("generic", N), N, L, dt, nu)
    try:
        run.rhs()
        r0 = run.norm(reference_form=True)
        assert run.cycle() > r0
    finally:
        run.close()

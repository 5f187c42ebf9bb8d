"""CPU: the conditions tests/test_gpu_bdf.py relies on, on the checker alone
(tests/bdf.py, tests/fields.py), and the formulas themselves.

Every case the GPU tests run against the checker (bdf.CASES) must stay finite,
converge under the cycle cap and keep every r_k / r_0 at least fields.MARGIN
(1 %) away from the tolerance, so that a cycle count never hinges on a
summation order.  This is a condition, not a measurement.  Measured with the
checker (tol 1e-9, seed 1; SEQ unless stated; cycles per step, smallest margin
over the steps):
  N=128  L=3 easy generic (bitwise, fma)    : 2,2,2,3,1,2,2,2  0.60
  N=128  L=3 easy generic0                  : 2,2,2,3,1,2,2,2  0.67
  N=128  L=3 easy generic, separable source + rings (None,0,None,1,None,2,None,None)
                                            : 2,2,2,3,1,2,2,2  0.72
                          (the same source without rings: 0.61)
  N=256  L=4 easy generic (fma)             : 2,2,2,3,1,2,2,2  0.59
  N=1024 L=6 easy generic (bitwise, fma)    : 2,2,2,2,1,2,2,2  0.16
  N=1024 L=6 easy generic, correct tower (fma): 2,2,2,2,1,2,2,2  0.15
  N=4096 L=7 easy generic (bitwise, fma)    : 2,2,2,3,2,2,2,2  0.74
  N=4096 L=7 easy rank1 (fma), SEQ_R1       : 2 every step     0.86
  N=4096 L=7 stiff generic (fma), SEQ_STIFF : 6,8,5,8,7,7      0.21
Avoided: rank1 at N=4096 with SEQ (its b2 step has margin 0.003).

The order check is the one that tells the variable-step coefficients from the
constant-step ones: on a grid of steps alternating 4/3 and 2/3 of the mean
(w alternating 1/2 and 2) constant-step coefficients fall to first order.
Smooth problem, N=64, L=3, u0 = sin(pi x) sin(2 pi y), the reference's rotating
flow, nu = -0.01, T = 0.1, tol 1e-13, errors against 4096 Crank-Nicolson steps,
n = 16, 32, 64, 128 steps; measured error ratios between successive n:
  implicit Euler 1.97, 1.99, 1.99;  Crank-Nicolson 3.99, 4.00, 4.00;
  BDF2 constant 3.80, 3.92, 3.97;   BDF2 alternating 3.81, 3.92, 3.97.
"""
import numpy as np
import pytest

import bdf as B
import fields as F


@pytest.fixture
def checker(oracle_mod):
    O = oracle_mod
    O.set_threads(16)
    yield O
    O.set_fp_mode(0)
    O.set_threads(1)


def test_constant_step_coefficients():
    for dt in (.1, 1.0 / 1280, 3e-5, 7.0):
        g, b0, b1, kA = B.coefs(dt, dt)
        assert g == np.float64(2.0) / np.float64(3.0)
        assert b0 == np.float64(4.0) / np.float64(3.0)
        assert b1 == np.float64(1.0) / np.float64(3.0)
        assert abs((b0 - b1) - 1.0) <= np.spacing(np.float64(1.0))
        assert kA == (np.float64(2.0) * g) * np.float64(dt)
    # consistency of the variable-step form, up to rounding: constants (b0 - b1
    # = 1) and u = t (dt - b1 dt_prev = g dt, that is b1 / w = 1 - g)
    for w in (.5, 2.0, .7, 1.5, 2.4):
        g, b0, b1, _ = B.coefs(w, 1.0)
        assert abs((b0 - b1) - 1.0) <= 4 * np.spacing(np.float64(1.0))
        assert abs(b1 / w - (1.0 - g)) <= 1e-15
    for seq in (B.SEQ, B.SEQ_R1, B.SEQ_STIFF):
        assert seq[0] == ("t", 1, .5)
        # zero-stability of every BDF2 step of the sequences: w < 1 + sqrt(2)
        for a, b in zip(seq, seq[1:]):
            if b[0] == "b":
                assert b[1] / a[1] < 1 + np.sqrt(2.0)


@pytest.mark.parametrize(B.CASE_ARGS, B.CASE_PARAMS, ids=B.CASE_IDS)
def test_no_cycle_norm_sits_at_the_tolerance(checker, N, L, pname, name, tower, fp, seq, extra,
                                             nsmooth, fuse, shape):
    O = checker
    O.set_fp_mode(fp)
    dt, nu = F.params(pname, N)
    run = F.CheckerRun(O, *F.make(name, N), N, L, dt, nu, tower, nsmooth, shape, fp)
    try:
        steps = B.checker_steps(run, dt, seq, B.TOL, B.T.source_field(N)[2] if extra else None,
                                B.RINGS if extra else None, keep_u=False)
        finite = bool(np.all(np.isfinite(run.u)))
    finally:
        run.close()
    print([(c, F.margin(r0, norms, B.TOL)) for c, r0, norms, _ in steps])
    assert finite
    for k, (cyc, r0, norms, _) in enumerate(steps):
        assert np.isfinite(r0) and np.all(np.isfinite(norms)), (k, r0, norms)
        assert cyc < 50 and norms[-1] / r0 <= B.TOL, (k, cyc, r0, norms)
        assert F.margin(r0, norms, B.TOL) >= F.MARGIN, (k, r0, norms)


# ---- the order of the schemes
ORDER_N, ORDER_L, ORDER_NU, ORDER_T, ORDER_TOL = 64, 3, -0.01, 0.1, 1e-13
ORDER_STEPS = (16, 32, 64, 128)


def _march(O, u0, v1, v2, dts, scheme):
    """u after the steps dts: scheme "cn" / "ie" theta-steps, "bdf2" a
    Crank-Nicolson start-up step then BDF2 steps."""
    N = ORDER_N
    run = F.CheckerRun(O, u0.copy(), v1, v2, N, ORDER_L, float(dts[0]), ORDER_NU, 0)
    try:
        h_prev, dt_prev = None, None
        for dt in dts:
            un = run.u.copy()
            if scheme == "bdf2" and h_prev is not None:
                g, b0, b1, kA = B.coefs(dt, dt_prev)
                B.bdf_rhs(run.t.rhsfine, un, h_prev, N, b0, b1)
            else:
                kA, kB = B.T.k_pair(dt, 1.0 if scheme == "ie" else .5)
                run.dt = float(kB)
                run.rhs()
            run.dt = float(kA)
            # (1e-13 is below what the smallest steps can reach: the cycle cap
            # ends those solves at rounding level)
            run.mg_outer(ORDER_TOL)
            h_prev, dt_prev = un, dt
        return run.u.copy()
    finally:
        run.close()


def test_variable_step_bdf2_is_second_order(checker):
    O = checker
    O.set_fp_mode(0)
    N = ORDER_N
    _, v1, v2 = O.init_problem(N)
    x = np.arange(N + 1) / N
    u0 = np.ascontiguousarray(np.sin(np.pi * x)[:, None] * np.sin(2 * np.pi * x)[None, :]).ravel()
    ref = _march(O, u0, v1, v2, [np.float64(ORDER_T) / 4096] * 4096, "cn")

    def grid(n, alternating):
        mean = np.float64(ORDER_T) / n
        if not alternating:
            return [mean] * n
        return [mean * (np.float64(4.0) / 3 if k % 2 == 0 else np.float64(2.0) / 3)
                for k in range(n)]

    def ratios(scheme, alternating=False):
        err = [np.max(np.abs(_march(O, u0, v1, v2, grid(n, alternating), scheme) - ref))
               for n in ORDER_STEPS]
        return [err[k] / err[k + 1] for k in range(len(err) - 1)]
    ie, cn = ratios("ie"), ratios("cn")
    bc, ba = ratios("bdf2"), ratios("bdf2", True)
    print("implicit Euler", ie, "Crank-Nicolson", cn, "BDF2 constant", bc, "BDF2 alternating", ba)
    assert all(r <= 2.2 for r in ie), ie
    assert all(r >= 3.5 for r in bc[-2:]), bc
    assert all(r >= 3.5 for r in ba[-2:]), ba

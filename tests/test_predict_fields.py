"""CPU: the conditions tests/test_gpu_predict.py relies on, on the checker alone
(tests/predict.py).

Every case the GPU tests run against the checker (predict.CASES) must stay
finite and under the cycle cap, keep every deciding ratio -- each r_k / r_0 and
the starting rp / r_0 -- at least fields.MARGIN (1 %) away from the tolerance,
and keep rp / r_0 at least that far from 1, so that neither a cycle count nor an
adoption hinges on a summation order.  Across the cases there must be adopted
and refused guesses, and the predictor must never cost a cycle.  These are
conditions, not measurements.  Measured with the checker (tol 1e-9, seed 1,
bdf.SEQ unless stated; total cycles over all steps for order 0 / the case's
order; rp / r_0 over the predicted steps; smallest margin of the predicted run):
  N=8    L=2 easy generic bitwise q1       : 13 / 12   0.12-0.30      0.69
  N=8    L=2 easy generic bitwise q2       : 13 / 11   0.03-0.21      0.67
  N=128  L=3 easy smooth  bitwise q1       : 12 / 10   0.016-0.042    0.066
  N=128  L=3 easy smooth  bitwise q2       : 12 / 10   0.003-0.029    0.066
  N=32   L=2 easy generic bitwise q2       : 15 / 14   0.02-0.13      0.10
  N=32   the same, reversed before step 3  : 13 / 13   refused at 6.05 0.13
  N=128  L=3 easy generic bitwise, fma q2  : 16 / 15   0.04-0.22      0.15
  N=128  the same, reversed before step 3  : 16 / 16   refused at 5.54 0.58
  N=128  separable source + rings, q2      : 16 / 16   0.05-0.53      0.47
         (the ring steps 1 and 3 run unpredicted)
  N=128  field source, fma q1              : 16 / 16   0.13-0.32      0.55
  N=1024 L=6 easy generic fma q1           : 15 / 15   0.16-0.45      0.16
  N=4096 L=7 easy rank1 fma q2, SEQ_R1     : 16 / 16   refused at 1.27, 1.51, 2.43,
                                             adopted at 0.60, 0.57, 0.19   0.27
  N=4096 L=7 stiff generic fma q2, SEQ_STIFF: 41 / 41  every guess refused, at
                                             4.39, 5.96, 3.49, 5.21        0.21
"""
import numpy as np
import pytest

import fields as F
import predict as P


@pytest.fixture
def checker(oracle_mod):
    O = oracle_mod
    O.set_threads(16)
    yield O
    O.set_fp_mode(0)
    O.set_threads(1)


_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _RUNS.clear()


def run(O, N, L, pname, name, fp, seq, order, extra):
    """(cyc, r0, norms, e, adopted, rp) per step, cached; u is not kept."""
    key = (N, L, pname, name, fp, seq, order, extra)
    if key not in _RUNS:
        O.set_fp_mode(fp)
        try:
            steps = P.run_case(O, N, L, pname, name, fp, seq, order, extra)
        finally:
            O.set_fp_mode(0)
        finite = all(bool(np.all(np.isfinite(s.u))) for s in steps)
        _RUNS[key] = (finite, [s._replace(u=None, un=None, h=None) for s in steps])
    return _RUNS[key]


@pytest.mark.parametrize(P.CASE_ARGS, P.CASES, ids=P.CASE_IDS)
def test_no_deciding_ratio_sits_at_its_threshold(checker, N, L, pname, name, fp, seq, order,
                                                 extra):
    finite, steps = run(checker, N, L, pname, name, fp, seq, order, extra)
    print([(s.cyc, s.e, int(s.adopted), None if s.rp is None else float(s.rp / s.r0),
            P.margin(s)) for s in steps])
    assert finite
    for k, s in enumerate(steps):
        assert np.isfinite(s.r0) and np.all(np.isfinite(s.norms)), (k, s.r0, s.norms)
        assert s.cyc < P.MAX_CYCLE and s.res / s.r0 <= P.TOL, (k, s.cyc, s.r0, s.norms)
        for r in P.ratios(s):
            assert abs(r / P.TOL - 1.0) >= F.MARGIN, (k, r)
        if s.e:
            assert np.isfinite(s.rp), (k, s.rp)
            assert abs(float(s.rp) / float(s.r0) - 1.0) >= F.MARGIN, (k, s.rp, s.r0)
            assert s.adopted == (s.rp < s.r0)
    # the effective orders: linear until u^(n-2) is resident, none on a ring step
    _, rings, _ = P.case_extra(extra, N)
    seen_b = 0
    for k, (s, st) in enumerate(zip(steps, seq)):
        ring = rings is not None and rings[k] is not None
        if st[0] != "b" or ring:
            assert s.e == 0, (k, s.e)
        else:
            assert s.e == (2 if order == 2 and k >= 2 else 1), (k, s.e)
        seen_b += st[0] == "b"
    assert seen_b


@pytest.mark.parametrize(P.CASE_ARGS, P.CASES, ids=P.CASE_IDS)
def test_the_predictor_never_costs_a_cycle(checker, N, L, pname, name, fp, seq, order, extra):
    _, plain = run(checker, N, L, pname, name, fp, seq, 0, extra)
    _, pred = run(checker, N, L, pname, name, fp, seq, order, extra)
    a, b = sum(s.cyc for s in plain), sum(s.cyc for s in pred)
    print("plain", [s.cyc for s in plain], "order", order, [s.cyc for s in pred])
    assert all(s.e == 0 for s in plain)
    assert b <= a, (a, b)
    if (N, L, pname, name, fp, seq, extra) in P.GAINS:
        assert b < a, (a, b)


@pytest.mark.parametrize("N,L,fp,depth", P.RETRY_CASES)
def test_the_retry_runs_keep_their_margins(checker, N, L, fp, depth):
    """Measured: smallest margin 0.78 at N=128 (either depth), 0.16 at N=1024
    depth 1 and 0.039 at N=1024 depth 2 (the step after the retry); effective
    orders of the tail 1, 2, 2 at depth 2 and 0, 1, 1 at depth 1."""
    O = checker
    dt, nu = F.params("easy", N)
    seq = P.RETRY_PREFIX + P.retry_tail(depth)
    O.set_fp_mode(fp)
    steps = P.checker_steps(O, *P.make("generic", N), N, L, dt, nu, seq, 2, depth, fp=fp,
                            linear_at=(len(P.RETRY_PREFIX),))
    print([(s.cyc, s.e, int(s.adopted), P.margin(s)) for s in steps])
    assert [s.e for s in steps[len(P.RETRY_PREFIX):]] == ([1, 2, 2] if depth == 2 else [0, 1, 1])
    for k, s in enumerate(steps):
        assert np.all(np.isfinite(s.u)) and s.cyc < P.MAX_CYCLE and s.res / s.r0 <= P.TOL, k
        assert P.margin(s) >= F.MARGIN, (k, s.r0, s.rp, s.norms)


def test_the_error_record_case_adopts_every_guess(checker):
    """tests/test_gpu_predict.py's step_error / dense case: (t1, b1, b1.5, b.5)
    at order 2 on generic, fma, N=128 and 1024."""
    O = checker
    seq = (P.B.t(1, .5), P.B.b(1), P.B.b(1.5), P.B.b(.5))
    for N, L in ((128, 3), (1024, 6)):
        dt, nu = F.params("easy", N)
        O.set_fp_mode(1)
        steps = P.checker_steps(O, *P.make("generic", N), N, L, dt, nu, seq, 2, 2, fp=1)
        O.set_fp_mode(0)
        print([(s.cyc, s.e, float(s.rp / s.r0) if s.e else None, P.margin(s)) for s in steps])
        assert [(s.e, s.adopted) for s in steps[1:]] == [(1, True), (2, True), (2, True)]
        assert all(P.margin(s) >= F.MARGIN for s in steps)


def test_adopted_and_refused_guesses_both_occur(checker):
    adopted = refused = 0
    for c in P.CASES:
        if c[0] > 128:
            continue
        _, steps = run(checker, *c)
        adopted += sum(1 for s in steps if s.e and s.adopted)
        refused += sum(1 for s in steps if s.e and not s.adopted)
    assert adopted > 0 and refused > 0, (adopted, refused)
    assert {c[:6] + (c[7],) for c in P.CASES} >= set(P.GAINS)
    for g in P.GAINS:
        assert {c[6] for c in P.CASES if c[:6] + (c[7],) == g} == {1, 2}, g

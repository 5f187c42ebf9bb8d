"""CPU: the conditions tests/test_gpu_schedules.py relies on, on the checker
alone (tests/schedules.py, tests/fields.py).

Every case of schedules.CASES that runs mg_outer (nsmooth >= 1) must stay
finite, converge under the cycle cap of 50 in its continued mg_outer and in
both steps, and keep every r_k / r_0 at least fields.MARGIN (1 %) away from its
tol, so that a cycle count never hinges on a summation order.  This is a
condition, not a measurement; no case is skipped.  The list must also keep
covering what schedules.check_coverage names.

Measured with the checker (seed 1): cycles of the continued mg_outer (after the
three cycles of the sequence) and of the two steps, the last r_k / r_0 of each,
the smallest margin of the three.  Case ids as schedules.case_id: N, L, params,
field, tower, fp mode, nsmooth / fuse, shape, form, parts; tol is 1e-9 where the
last ratios are below 1e-9, else 1e-6.
  N128-L1-easy5-generic-t0-bitwise-s3f3-V-tiles      8,2,2   2.9e-07 5.0e-07 4.9e-07  0.50
  N128-L1-visc16-generic0-t1-bitwise-s2f2-W-march    13,1,1  5.3e-07 1.8e-07 2.6e-07  0.47
  N128-L2-visc07-generic-t0-fma-s3f3-W-tiles         4,3,3   7.0e-09 5.3e-07 2.7e-07  0.47
  N128-L2-easy3-rank1-t1-bitwise-s1f1-V-march        4,4,4   4.8e-08 1.8e-08 3.8e-08  0.15
  N128-L3-visc07-generic-t0-bitwise-s3f3-W-tiles     4,3,3   7.0e-09 5.3e-07 2.7e-07  0.47
  N128-L3-visc16-generic-t0-fma-s2f1-V-tiles         8,7,7   2.5e-07 4.3e-07 6.2e-07  0.38
  N128-L3-visc06-rank1-t1-fma-s1f3-W-march           6,6,6   2.8e-10 1.8e-10 3.7e-10  0.63
  N128-L3-visc07-generic-t1-bitwise-s4f3-V-tiles     5,5,4   6.1e-07 8.7e-08 7.5e-07  0.25
  N256-L8-visc16-generic-t0-bitwise-s3f3-V-tiles     5,4,5   2.9e-07 8.3e-07 6.2e-08  0.17
  N256-L8-visc16-rank1-t1-fma-s2f2-W-march           6,5,5   2.3e-10 3.6e-10 4.8e-10  0.52
  N256-L8-visc16-generic0-t0-fma-s2f3-V-mixed        8,7,7   2.1e-07 2.9e-07 4.3e-07  0.40
  N256-L7-visc16-generic-t1-bitwise-s3f3-W-tiles     3,2,3   4.0e-07 7.9e-07 2.9e-09  0.20
  N256-L7-easy3-generic-t0-fma-s1f1-V-mixed          8,7,7   3.8e-07 6.6e-07 4.9e-07  0.34
  N256-L7-visc16-generic-t0-bitwise-s3f2-W-mixed     3,2,3   3.8e-07 8.3e-07 3.1e-09  0.17
  N256-L4-visc30-generic-t0-fma-s3f3-W-mixed         7,6,6   8.4e-11 7.3e-11 9.3e-11  0.36
  N256-L4-visc16-generic-t1-fma-s3f3-V-mixed         5,4,5   2.8e-07 8.0e-07 5.9e-08  0.20
  N256-L4-visc06-generic0-t0-bitwise-s4f3-W-tiles    5,6,6   5.8e-07 1.3e-07 2.2e-07  0.29
  N256-L4-visc16-rank1-t0-bitwise-s2f2-V-march       8,6,7   2.1e-07 8.6e-07 1.8e-07  0.14
  N256-L3-visc16-generic-t0-bitwise-s3f3-V-march     5,4,5   2.9e-07 8.3e-07 6.1e-08  0.17
  N256-L3-visc16-generic-t1-fma-s2f2-W-tiles         4,4,4   2.2e-07 3.0e-08 4.5e-08  0.37
  N256-L3-visc30-rank1-t0-fma-s4f3-W-march           5,4,4   1.8e-10 2.5e-10 3.0e-10  0.70
  N256-L2-visc16-generic-t0-fma-s3f1-V-tiles         4,4,5   5.7e-07 8.1e-07 2.7e-08  0.19
  N256-L2-visc07-generic0-t1-bitwise-s3f3-W-march    4,3,3   1.2e-07 6.7e-07 8.3e-07  0.17
  N512-L5-visc07-generic-t0-bitwise-s3f3-W-march     5,4,4   4.6e-08 7.4e-08 9.4e-08  0.37
  N512-L5-visc16-generic-t0-fma-s3f3-V-tiles         5,4,4   2.7e-07 4.8e-07 6.8e-07  0.32
  N512-L5-easy3-generic0-t1-bitwise-s1f2-W-mixed     4,3,3   8.2e-08 6.5e-07 7.1e-07  0.29
  N512-L5-visc16-rank1-t0-fma-s4f3-V-mixed           6,5,5   7.3e-11 5.7e-11 8.3e-11  0.52
  N512-L4-visc30-rank1-t1-bitwise-s3f3-W-mixed       7,5,5   8.1e-10 6.9e-10 8.6e-10  0.14
  N512-L4-easy3-generic-t0-fma-s2f2-V-march          4,3,3   1.0e-07 6.3e-07 6.8e-07  0.32
  N512-L4-visc16-generic-t0-bitwise-s2f1-W-tiles     4,3,4   2.7e-07 9.0e-07 2.7e-08  0.10
  N512-L4-easy5-generic-t0-fma-s1f1-V-tiles          6,6,6   2.4e-10 4.1e-11 4.3e-11  0.76
  N512-L3-visc16-generic-t0-bitwise-s3f3-V-tiles     5,4,4   2.7e-07 4.8e-07 6.8e-07  0.32
  N512-L3-visc07-generic-t0-fma-s2f3-W-march         7,6,6   2.8e-07 1.7e-07 1.9e-07  0.45
  N512-L3-easy3-generic0-t1-fma-s1f3-W-tiles         4,3,3   8.2e-08 6.5e-07 7.1e-07  0.29
  N512-L3-visc07-generic-t1-bitwise-s4f3-V-march     7,5,5   1.3e-07 4.6e-07 5.9e-07  0.30
  N2048-L3-stiff-generic-t0-fma-s3f3-V-march         8,7,7   2.8e-10 2.0e-10 2.6e-10  0.72
  N2048-L3-visc07-generic-t0-bitwise-s3f3-W-tiles    5,4,4   8.5e-08 7.3e-08 9.3e-08  0.91
  N2048-L6-stiff-generic-t1-fma-s2f2-W-mixed         4,3,3   2.7e-07 5.7e-07 7.1e-07  0.29
  N2048-L6-visc16-rank1-t0-bitwise-s4f3-V-mixed      4,3,3   5.5e-08 1.5e-07 1.7e-07  0.83
  N1024-L5-visc07-generic-t0-fma-s3f3-W-tiles-p2     5,4,4   6.4e-08 5.8e-08 7.5e-08  0.67
  N1024-L5-visc07-generic-t0-bitwise-s4f3-V-mixed-p2 7,5,5   1.4e-07 4.3e-07 5.5e-07  0.29
  N1024-L5-easy5-generic-t1-fma-s1f1-V-march-p2      4,4,4   9.0e-08 4.7e-08 5.0e-08  0.91
Avoided (why the params differ from case to case): three cycles run before the
mg_outer, so with "visc16" the W-cycles with nsmooth >= 3 have reached the
rounding floor (r / r_0 ~ 5e-16) by then and the continued mg_outer runs into
the cap; W-cycles on rank1 contract faster still and take "visc30"; nsmooth 1
V-cycles with any "visc" set need 20-35 cycles; "easy3" with nsmooth 1 at
N=512, L=4 and at N=1024 has a norm within 0.3 % / 3 % of 1e-6; "stiff"
diverges below N = 2048 (tests/test_fields.py).  The N = 4096 W-cycle case is
checked in tests/test_fields.py's way by tests/test_gpu_generic_fields.py
itself (margins_ok): a checker run of that size takes 13-17 s on 16 threads, a
third of this whole file (43 s).
"""
import numpy as np
import pytest

import fields as F
import schedules as S


@pytest.fixture
def checker(oracle_mod):
    O = oracle_mod
    O.set_threads(16)
    yield O
    O.set_fp_mode(0)
    O.set_threads(1)


def test_the_list_covers_what_it_must():
    assert S.check_coverage() == []
    assert len(set(S.CASE_IDS)) == len(S.CASES)
    small = [c for c in S.CASES if c.N in (128, 256, 512)]
    assert 35 <= len(small) <= 45
    assert all(c.N in (128, 256, 512, 2048) or (c.N == 1024 and c.parts == 2) for c in S.CASES)
    assert all(c.tol in (1e-6, 1e-9) and c.params in F.PARAMS and c.form in S.FORMS
               for c in S.CASES)
    # the check itself notices a thinned list
    assert S.check_coverage([c for c in S.CASES if c.nsmooth != 4])
    assert S.check_coverage([c for c in S.CASES if not (c.shape == 2 and S.coarsest_n(c) == 64)])
    assert S.check_coverage([c for c in S.CASES if not c.parts])


def test_forms_put_the_levels_where_the_docstring_says():
    c = S.CASES[0]._replace(N=512, L=5)
    assert S.level_forms(c._replace(form="tiles")) == ["tiles"] * 4
    assert S.level_forms(c._replace(form="march")) == ["march"] * 4
    assert S.level_forms(c._replace(form="mixed")) == ["march", "march", "tiles", "tiles"]
    assert S.coarsest_n(c) == 32


@pytest.mark.parametrize("case", [c for c in S.CASES if S.converges(c)],
                         ids=[S.case_id(c) for c in S.CASES if S.converges(c)])
def test_no_cycle_norm_sits_at_the_tolerance(checker, case):
    O = checker
    O.set_fp_mode(case.fp)
    run = S.checker_run(O, case, *F.make(case.field, case.N))
    try:
        want = S.checker_sequence(run, case)
    finally:
        run.close()
    outs = S.outers(want)
    print([(len(n), "%.1e" % (n[-1] / r0), round(F.margin(r0, n, case.tol), 2)) for r0, n in outs],
          want["its"])
    assert np.all(np.isfinite(want["us"]))
    for k, (r0, norms) in enumerate(outs):
        assert np.isfinite(r0) and np.all(np.isfinite(norms)), (k, r0, norms)
        assert len(norms) < 50 and norms[-1] / r0 <= case.tol, (k, r0, norms)
        assert F.margin(r0, norms, case.tol) >= F.MARGIN, (k, r0, norms)


@pytest.mark.parametrize("case", [c for c in S.CASES if not S.converges(c)],
                         ids=[S.case_id(c) for c in S.CASES if not S.converges(c)])
def test_unsmoothed_cycles_stay_finite(checker, case):
    """nsmooth 0: three cycles of restriction, coarsest solve and prolongation
    only; nothing converges, nothing may overflow."""
    O = checker
    O.set_fp_mode(case.fp)
    run = S.checker_run(O, case, *F.make(case.field, case.N))
    try:
        want = S.checker_sequence(run, case)
    finally:
        run.close()
    assert "outer" not in want
    assert np.all(np.isfinite(want["u3"])) and np.all(np.isfinite(want["norms"]))
    assert want["its3"] > 0

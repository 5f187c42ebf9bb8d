"""mgx_set_source / Multigrid.set_source: u_t + v.grad u = nu lap u + f.

The contract (include/mgx.h): with a source f and a scale s every finest-level
compute_rhs of the context gives, on the interior,
    rhs = fl( Bu + fl( c * f ) ),   c = fl(dt * s),
Bu being the homogeneous compute_rhs.  That is exact, so the bar is BITWISE:
the expected values are the CPU checker's compute_rhs plus the term added with
numpy (which rounds the product, then the sum), its mg_outer on that rhs, and
equal cycle counts.  Norms taken by different kernels agree to 1e-11 relative
(the bound mgx.h documents); the initial norm of a step is bitwise the norm of
rhs() + residual_norm(0).

The source is an off-centre Gaussian emitter with a ripple: with dt = 1/N/10
and nu = 4e-4 it moves u by 0.046 (N=256), 0.012 (N=1024) and 0.017 (N=4096)
over three steps, so no test passes by ignoring it.  Cycle counts of the checker
(run on the CPU before these tests were written): 1 per step at tol 1e-6 for
N=256/L=4 (both towers) and N=1024/L=6; 2 per step at tol 1e-6 for N=4096/L=7
(3 per step from tol 1e-8 on), so N=4096 runs at 1e-6 and asserts >= 2.
"""
import numpy as np
import pytest
import torch   # before libmgx loads: one HIP runtime in the process

from hpcclassmultigridproject_amd import Multigrid, _lib, init_problem

pytestmark = pytest.mark.gpu
NU = 4e-4
NORM_RTOL = 1e-11
DEV = "cuda:0"


def make_source(N, shift=0.0):
    x = (np.arange(N + 1) / N)[:, None]
    y = (np.arange(N + 1) / N)[None, :]
    f = (50.0 * np.exp(-200.0 * ((x - .7 + shift) ** 2 + (y - .3) ** 2))
         * (1.0 + .5 * np.sin(7 * x + 3 * y)))
    return np.ascontiguousarray(f).ravel()


def interior(N):
    m = np.zeros((N + 1, N + 1), bool)
    m[1:N, 1:N] = True
    return m.ravel()


def bits(a):
    return a.view(np.uint64)


_problems = {}


def problem(N):
    """(u0, v1, v2, f) of size N, made once and never modified."""
    if N not in _problems:
        p = init_problem(N) + (make_source(N),)
        for a in p:
            a.setflags(write=False)
        _problems[N] = p
    return _problems[N]


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


# ---------------------------------------------------------------- 1. the raw op
@pytest.mark.parametrize("n", [2, 4, 8, 64, 512, 1024])
def test_raw_op_bitwise_vs_numpy(oracle_mod, n):
    """n=2: one interior point; n=512: column n alone in a second 512-column
    strip of the context kernel's frame (the raw op has one lane per point)."""
    O = oracle_mod
    rng = np.random.default_rng(n)
    cnt = (n + 1) ** 2
    u, v1, v2, f = (rng.uniform(-2, 2, cnt) for _ in range(4))
    c = float(rng.uniform(-2, 2))
    k, nu, h = 0.1 / n, -0.01, 1.0 / n
    sentinel = 7.25
    want = np.full(cnt, sentinel)
    inr = interior(n)
    bu = O.compute_rhs(u, n, v1, v2, k, nu, h)
    want[inr] = bu[inr] + c * f[inr]
    rhs = torch.full((cnt,), sentinel, dtype=torch.float64, device=DEV)
    dev = [torch.from_numpy(a).to(DEV) for a in (u, v1, v2, f)]
    _lib.compute_rhs_source(rhs, dev[0], n, dev[1], dev[2], k, nu, h, dev[3], c)
    torch.cuda.synchronize()
    got = rhs.cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(got[inr], bu[inr])


# ------------------------------------------------------- 2. steps vs the checker
def oracle_steps(O, N, L, tower, steps, tol, s=1.0):
    u0, v1, v2, f = problem(N)
    dt = 1.0 / N / 10
    inr = interior(N)
    t = O.Tower(u0, v1, v2, N, L, tower)
    cyc = []
    for _ in range(steps):
        rhs = O.compute_rhs(t.ufine, N, v1, v2, dt, NU, 1.0 / N)
        rhs[inr] += dt * s * f[inr]
        t.rhsfine[:] = rhs
        cyc.append(t.mg_outer(dt, NU, tol)[0])
    return t.ufine.copy(), cyc


def gpu_steps(N, L, tower, steps, tol, s=1.0, fp=_lib.FP_BITWISE, **kw):
    u0, v1, v2, f = problem(N)
    with Multigrid(N, L, 1.0 / N / 10, NU, tower_mode=tower, fp_mode=fp, **kw) as mg:
        mg.upload(u0, v1, v2)
        mg.set_source(f)
        if s != 1.0:
            mg.set_source_scale(s)
        out = [mg.step_ex(tol) for _ in range(steps)]
        return mg.download(), [o[0] for o in out], [o[1:] for o in out]


@pytest.mark.parametrize("N,L,tower,s,mincyc", [
    (256, 4, _lib.TOWER_REFERENCE, 1.0, 1),   # LDS-tile levels only
    (256, 4, _lib.TOWER_CORRECT, 0.75, 1),    # and a scale: c = fl(dt * s)
    (1024, 6, _lib.TOWER_REFERENCE, 1.0, 1),
    (4096, 7, _lib.TOWER_REFERENCE, 1.0, 2),  # row march + cross-cycle schedule
], ids=["N256-reference", "N256-correct-scaled", "N1024", "N4096"])
def test_steps_bitwise_vs_oracle(oracle_mod, N, L, tower, s, mincyc):
    O = oracle_mod
    O.set_threads(16)
    try:
        want, cyc_ref = oracle_steps(O, N, L, tower, 3, 1e-6, s)
    finally:
        O.set_threads(1)
    assert min(cyc_ref) >= mincyc, cyc_ref
    got, cyc, _ = gpu_steps(N, L, tower, 3, 1e-6, s)
    assert cyc == cyc_ref
    assert np.array_equal(bits(got), bits(want))
    # (and the homogeneous equation would not have given this)
    assert float(np.max(np.abs(want - problem(N)[0]))) > 5e-3


def test_steps_fma_bitwise_vs_fma_checker(oracle_mod):
    """fp_mode fma: the smoothing passes contract, compute_rhs and the source
    term never do -- bit for bit the checker's fma form (tests/test_gpu_fma.py's
    comparison) on the same composed rhs."""
    O = oracle_mod
    N, L = 1024, 6
    O.set_threads(16)
    O.set_fp_mode(1)
    try:
        want, cyc_ref = oracle_steps(O, N, L, _lib.TOWER_REFERENCE, 3, 1e-6)
    finally:
        O.set_fp_mode(0)
        O.set_threads(1)
    got, cyc, _ = gpu_steps(N, L, _lib.TOWER_REFERENCE, 3, 1e-6, fp=_lib.FP_FMA)
    assert cyc == cyc_ref
    assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------ 3. the initial norm
@pytest.mark.parametrize("factors", [True, False], ids=["factors", "no-factors"])
@pytest.mark.parametrize("sv", [0, 1], ids=["sv0", "sv1"])
def test_initial_norm_is_rhs_then_residual_norm(knobs, factors, sv):
    """step's res0 (the norm instance of the source pass) == rhs() followed by
    residual_norm(0) (k_res_march<0> on the stored rhs) on a second context."""
    N, L = 4096, 7
    u0, v1, v2, f = problem(N)
    knobs(source_sv=sv, sep_velocity=1 if factors else 0)
    res = []
    for use_step in (True, False):
        with Multigrid(N, L, 1.0 / N / 10, NU) as mg:
            mg.upload(u0, v1, v2)
            assert (mg.velocity_factored() & 1) == (1 if factors else 0)
            mg.set_source(f)
            if use_step:
                res.append(mg.step_ex(1e-6)[1])
            else:
                mg.rhs()
                res.append(mg.residual_norm(0))
    assert res[0] > 0
    assert np.float64(res[0]).view(np.uint64) == np.float64(res[1]).view(np.uint64), res


# ---------------------------------------------------------- 4. the factor variant
def test_factor_variant_bitwise_and_bytes(knobs):
    N, L = 4096, 7
    u0, v1, v2, f = problem(N)
    out = []
    for sv in (0, 1):
        knobs(source_sv=sv)
        with Multigrid(N, L, 1.0 / N / 10, NU, fp_mode=_lib.FP_FMA) as mg:
            mg.upload(u0, v1, v2)
            assert mg.velocity_factored() & 1
            mg.set_source(f)
            mg.profile(True)
            steps = [mg.step_ex(1e-6) for _ in range(2)]
            mg.rhs()   # the rhs-only instance as well
            rhs = mg.download_level(0, "rhs")
            n, _, b, cb = mg.profile_get_ex(_lib.K_RHS, 0)
            out.append((steps, mg.download(), rhs, n, b, cb))
    (s0, u_0, r0, n0, b0, cb0), (s1, u_1, r1, n1, b1, cb1) = out
    assert s0 == s1   # cycles, res0, res: bitwise
    assert np.array_equal(bits(u_0), bits(u_1))
    assert np.array_equal(bits(r0), bits(r1))
    assert n0 == n1 == 3 and b0 == b1
    M = float((N + 1) ** 2)
    assert cb0 == 3 * 40.0 * M            # u, v1, v2, f read, rhs written
    assert cb0 - cb1 == 3 * 16.0 * M      # exactly the two velocity streams


# ------------------------------------------------- 5. the fused-schedule interplay
# nu = +4e-4 (the value of the checker comparisons above) does not converge at
# N=8192: mg_outer hits its 50-cycle cap with or without a source (2 cycles per
# step at N=4096, 1 below).  This GPU-against-GPU test uses the value every
# other test of the project runs, -4e-4, and asserts that every step converged.
NU_LARGE = -4e-4


def _interplay(N, L, f):
    u0, v1, v2, _ = problem(N)
    us, cyc = [], []
    with Multigrid(N, L, 1.0 / N / 10, NU_LARGE) as mg:
        mg.upload(u0, v1, v2)
        for act in (None, lambda: mg.set_source(f), lambda: mg.set_source_scale(0.5),
                    lambda: mg.set_source(None)):
            if act:
                act()
            cyc.append(mg.step(1e-6))
            us.append(mg.download())
    return us, cyc


def test_fused_schedule_interplay(knobs):
    """N=8192, L=8: step-cross engages (a pending next step when the source
    arrives, changes scale and leaves).  GPU against GPU: the unfused schedule
    is what test_steps_bitwise_vs_oracle pins to the checker."""
    N, L = 8192, 8
    u0, v1, v2, f = problem(N)
    ua, ca = _interplay(N, L, f)
    knobs(step_cross=0, step_fuse=0, cross_cycle=0)
    ub, cb = _interplay(N, L, f)
    assert ca == cb and 1 <= min(ca) and max(ca) < 50
    for a, b in zip(ua, ub):
        assert np.array_equal(bits(a), bits(b))
    # the source acted, the scale acted ...
    knobs(step_cross=1, step_fuse=1, cross_cycle=1)
    with Multigrid(N, L, 1.0 / N / 10, NU_LARGE) as mg:
        mg.upload(ua[0], v1, v2)
        mg.step(1e-6)
        plain = mg.download()
        assert float(np.max(np.abs(plain - ua[1]))) > 1e-4
        assert float(np.max(np.abs(ua[2] - ua[1]))) > 1e-4
        # ... and after set_source(None) the context is one that never had one
        # (download + upload, the equivalence set_velocity documents)
        mg.upload(ua[2], v1, v2)
        c3 = mg.step(1e-6)
        assert c3 == ca[3]
        assert np.array_equal(bits(mg.download()), bits(ua[3]))


# ------------------------------------------------------------------ 6. partitioned
@pytest.mark.parametrize("N,L,parts", [(1024, 4, 2), (1024, 4, 4), (256, 4, 2)],
                         ids=["N1024-2", "N1024-4", "N256-2-replicated"])
def test_partitioned_equals_single(N, L, parts):
    u0, v1, v2, f = problem(N)
    out = []
    for p in (0, parts):
        with Multigrid(N, L, 1.0 / N / 10, NU, local_parts=p) as mg:
            if p:
                assert (mg.dist_info()[2] == 0) == (N == 256)
            mg.upload(u0, v1, v2)
            mg.set_source(f)
            steps = [mg.step_ex(1e-6)]
            mg.set_source_scale(0.5)
            steps.append(mg.step_ex(1e-6))
            mg.rhs()
            steps.append((0, mg.residual_norm(0), 0.0))
            assert mg.source_info() == (True, 0.5)
            mg.set_source(None)
            steps.append(mg.step_ex(1e-6))
            out.append((mg.download(), steps))
    (us, ss), (up, sp) = out
    assert [s[0] for s in ss] == [s[0] for s in sp]
    assert np.array_equal(bits(us), bits(up))
    np.testing.assert_allclose([s[1] for s in sp], [s[1] for s in ss], rtol=NORM_RTOL)
    np.testing.assert_allclose([s[2] for s in sp], [s[2] for s in ss], rtol=NORM_RTOL)


# ------------------------------------------------------- 7. persistence and errors
def _fresh(N, L, u, v1, v2, f, steps=1, s=1.0):
    with Multigrid(N, L, 1.0 / N / 10, NU) as mg:
        mg.upload(u, v1, v2)
        if f is not None:
            mg.set_source(f)
            mg.set_source_scale(s)
        cyc = [mg.step(1e-6) for _ in range(steps)]
        return mg.download(), cyc


def test_persistence_replacement_and_errors():
    N, L = 256, 4
    u0, v1, v2, f = problem(N)
    g = make_source(N, shift=0.3)
    with Multigrid(N, L, 1.0 / N / 10, NU) as mg:
        assert mg.source_info() == (False, 1.0)
        mg.upload(u0, v1, v2)
        mg.set_source(torch.from_numpy(f.copy()).to(DEV))   # the device-pointer entry
        mg.set_source_scale(1.5)
        assert mg.source_info() == (True, 1.5)
        c1 = mg.step(1e-6)
        ua = mg.download()
        want, cw = _fresh(N, L, u0, v1, v2, f, s=1.5)
        assert [c1] == cw and np.array_equal(bits(ua), bits(want))
        # survives an upload ...
        mg.upload(u0, v1, v2)
        assert mg.source_info() == (True, 1.5)
        assert mg.step(1e-6) == c1
        assert np.array_equal(bits(mg.download()), bits(want))
        # ... and a new velocity
        mg.set_velocity(-v1, -v2)
        assert mg.source_info() == (True, 1.5)
        c2 = mg.step(1e-6)
        want2, cw2 = _fresh(N, L, want, -v1, -v2, f, s=1.5)
        assert [c2] == cw2 and np.array_equal(bits(mg.download()), bits(want2))
        # a different field replaces it
        mg.set_source(g)
        c3 = mg.step(1e-6)
        want3, cw3 = _fresh(N, L, want2, -v1, -v2, g, s=1.5)
        assert [c3] == cw3 and np.array_equal(bits(mg.download()), bits(want3))
        other, _ = _fresh(N, L, want2, -v1, -v2, f, s=1.5)
        assert not np.array_equal(want3, other)
        # rejected calls leave the context as it was
        lib = _lib.lib()
        assert lib.mgx_set_source(None, g.ctypes.data) == _lib.MGX_E_ARG
        assert "mgx_set_source" in lib.mgx_last_error().decode()
        assert lib.mgx_set_source_scale(None, 2.0) == _lib.MGX_E_ARG
        with pytest.raises(ValueError):
            mg.set_source(g[:-1].copy())
        assert mg.source_info() == (True, 1.5)
        c4 = mg.step(1e-6)
        want4, cw4 = _fresh(N, L, want3, -v1, -v2, g, s=1.5)
        assert [c4] == cw4 and np.array_equal(bits(mg.download()), bits(want4))
        # removed: the homogeneous step again
        mg.set_source(None)
        assert mg.source_info() == (False, 1.5)
        c5 = mg.step(1e-6)
        want5, cw5 = _fresh(N, L, want4, -v1, -v2, None)
        assert [c5] == cw5 and np.array_equal(bits(mg.download()), bits(want5))

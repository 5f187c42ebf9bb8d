"""The fused passes against the CPU checker on fields that are not
init_problem (tests/fields.py): O(1) noisy u with non-zero Dirichlet data, a
non-separable velocity that is non-zero on the boundary, and a synthetic
rank-1 flow whose factors are not the rotating flow's.

Bar, everywhere: u as uint64 equals the checker's u (the checker in the
matching fp mode), cycle counts are equal, norms agree to rtol 1e-11 (the
bound include/mgx.h documents for the tree summation).  The contract for the
boundary of u is the reference's: the ring is data -- read, never written
(multigrid.cpp:69-88 adds a prolongation that is zero there) -- so whole
arrays are compared, ring included.

Every checker computation runs once per (sequence, field, params, N, L, tower,
nsmooth, shape, fp) and is cached for the module; every knob variant compares
against that one result.  Before a cycle count is compared, the checker's own
norms must be at least 1 % away from the tolerance (fields.margin), so a
count never hinges on a summation order.

Where the library has an observable for a path, the test asserts it, so a
silent fallback fails: launch counts of the cross pass (cross_cycle), of the
rhs + norm pass (step_cross: one over all steps) and of the finest level's
pre-smoothing passes (step_fuse: one per step fewer), graph capture / replay
counters, factor masks (sep_velocity, vgen) and the partition info.  xfast,
xtile_max_rows, zero_rows, post_predict and post_only have no counter: for
those the proof is only that the key reads back as set and that the cross
pass ran.  (At N=4096 a whole level has 4097 rows, the default
xtile_max_rows, so the default run already takes its edges as LDS tiles --
k_xtile; xtile_max_rows=8193 repeats that, xtile_max_rows=0 is the variant
that runs the guarded edge march next to the unguarded interior kernel.)

The continued mg_outer of the cycle sequence runs to 1e-6, not 1e-9: after
four stiff cycles r_4 / r_0 = 2.7e-7, and 1e-9 of that is 2.7e-16 r_0 -- below
the residual's rounding floor (measured with the checker at N=4096, L=5:
5.2e-16 r_0 in bitwise mode from cycle 11 on), where it would stagnate to the
50-cycle cap.  1e-6 takes 5 more cycles (r_8, r_9 = 6.2 and 0.32 x the
threshold) and ends two decades above the floor.  The fresh mg_outer and the
time steps run to 1e-9.

Norms are compared with the accurately summed norm of the checker's residual
(fields.Norm.exact), not with the checker's serial sum: on these fields the
serial loop is itself 1.4e-11 / 1.5e-10 (two easy steps, N=8192) and 3.0e-11
(W-cycles, N=4096) off math.fsum of the same squares, where the solver's
tree sums are within 1.8e-16 of it.

Checker figures (seed 1; r_k / r_0 per cycle, smallest distance from the
threshold as fields.margin):
  generic, stiff, N=4096 L=5, reference tower, both fp modes: r_0 = 1535,
    6 cycles: 3.79e-3 1.33e-4 5.75e-6 2.69e-7 1.31e-8 6.50e-10 (margin 0.35);
    steps 2 and 3: 6 cycles each, last 7.70e-10 and 8.90e-10 (0.23, 0.11);
    continued: 5 cycles from r_4 = 4.12e-4 (0.68)
  correct tower: 6 cycles, last 4.64e-10 (0.54); continued 5 (0.72)
  nsmooth 2, L=4: 10 cycles, last 3.65e-10 (0.64); continued 8 (0.66)
  W-cycles, L=4: 3 cycles: 1.33e-4 2.68e-7 6.49e-10 (0.35); continued 3 from
    r_2 = 4.12e-4: 2.4e-3 6.3e-6 1.7e-8 (0.98)
  generic(boundary=False): 6 cycles, last 7.60e-10 (0.24); continued 5 (0.67)
  generic, easy, N=8192 L=6, bitwise: 2 cycles per step: 8.6e-6 2.2e-10 and
    7.2e-6 1.8e-10 (0.78, 0.82)
  rank1, stiff, N=4096 L=7: 6 cycles per step, last 5.3e-10 and 6.0e-10
    (reference tower; 0.47, 0.40), 5.1e-10 and 5.8e-10 (correct; 0.49, 0.42)
The file takes 55 s on one MI355X, most of it the checker (16 CPU threads
available, 8 used); the slowest case, marked slow, 7.4 s.
"""
import numpy as np
import pytest
import torch

import fields as F
from hpcclassmultigridproject_amd import Multigrid, _lib

pytestmark = pytest.mark.gpu
NORM_RTOL = 1e-11
TOL = F.TOL
TOL_CONTINUED = 1e-6
SEED = F.SEED
REF, CORRECT = _lib.TOWER_REFERENCE, _lib.TOWER_CORRECT
BITWISE, FMA = _lib.FP_BITWISE, _lib.FP_FMA

_FIELDS = {}
_CHECKER = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    """The cached fields and checker results (full grids, several GB in all)
    live for this module only."""
    yield
    _FIELDS.clear()
    _CHECKER.clear()


def field(name, N):
    """(u0, v1, v2) of fields.make, generated once per module and read-only."""
    if (name, N) not in _FIELDS:
        arrs = F.make(name, N, SEED)
        for a in arrs:
            a.setflags(write=False)
        _FIELDS[name, N] = arrs
    return _FIELDS[name, N]


def checker(O, seq, name, pname, N, L, tower=REF, nsmooth=3, shape=1, fp=BITWISE):
    """The cached checker result of sequence `seq` (one of the seq_* below)."""
    key = (seq.__name__, name, pname, N, L, tower, nsmooth, shape, fp)
    if key not in _CHECKER:
        dt, nu = F.params(pname, N)
        O.set_threads(8)
        O.set_fp_mode(fp)
        try:
            run = F.CheckerRun(O, *field(name, N), N, L, dt, nu, tower, nsmooth, shape, fp)
            try:
                _CHECKER[key] = seq(run)
            finally:
                run.close()
        finally:
            O.set_fp_mode(0)
            O.set_threads(1)
    return _CHECKER[key]


def bits_equal(got, want, N, what):
    """uint64 equality of two (N+1)^2 arrays; on failure say where they differ."""
    g, w = got.view(np.uint64), want.view(np.uint64)
    if np.array_equal(g, w):
        return
    bad = (g != w).reshape(N + 1, N + 1)
    rows, cols = np.nonzero(bad)
    ring = bad[0].sum() + bad[N].sum() + bad[1:N, 0].sum() + bad[1:N, N].sum()
    err = np.abs(got - want).reshape(N + 1, N + 1)[bad]
    raise AssertionError(
        f"{what}: {bad.sum()} of {bad.size} entries differ ({ring} on the ring), rows "
        f"{rows.min()}..{rows.max()}, columns {cols.min()}..{cols.max()}, first at "
        f"({rows[0]}, {cols[0]}), max |diff| {np.nanmax(err):.3e}")


def norms_close(got, want, what):
    """Against the accurately summed norm of the checker's residual
    (fields.Norm: the checker's serial sum is itself up to 1.5e-10 off)."""
    want = [w.exact for w in (want if isinstance(want, (list, tuple)) else [want])]
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.shape == want.shape, (what, got, want)
    rel = np.abs(got - want) / np.abs(want)
    assert np.all(rel <= NORM_RTOL), (what, got.tolist(), want.tolist(), rel.tolist())


def margins_ok(*outers):
    """Each (r0, norms, tol) of the checker keeps MARGIN from its threshold."""
    for r0, norms, tol in outers:
        assert len(norms) < 50 and norms[-1] / r0 <= tol, (r0, norms, tol)
        assert F.margin(r0, norms, tol) >= F.MARGIN, (r0, norms, tol)


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


def dev(a):
    return torch.from_numpy(np.array(a)).to("cuda:0")   # (a copy: the cached fields are read-only)


# ---------------------------------------------------------------- a. level passes

SMOOTHERS = [(0, 3), (0, 2), (0, 1), (1, 3), (2, 3)]   # tests/test_gpu_ops.py


@pytest.fixture(params=[(2048, 1 << 30, 0, None), (2048, 0, 1, None), (0, 1 << 30, 0, 0)],
                ids=["tile", "tile32xcd", "march"])
def tile_mode(request):
    """tests/test_gpu_ops.py: small levels as 2-D LDS tiles (16-row; or 32-row
    tiles in XCD order) or as the row march -- tile_max_n = 0 and
    march_tile_rows = 0, without which levels this short fall back to tiles
    (smooth_as_tiles).  The march's strips are 116 columns wide for three
    sweeps (WCfg::W; 124 for one, 112 with a residual stage): N=512 is five strips, the last group of four
    part-empty, N=128 two strips and its level 1 (n = 64) narrower than one;
    the level ops launch the guarded form over the whole level."""
    keys = ("tile_max_n", "tile32_min_n", "tile_xcd", "march_tile_rows")
    old = [_lib.get_tuning(k) for k in keys]
    for k, v in zip(keys, request.param):
        if v is not None:
            _lib.set_tuning(k, v)
    yield request.param[0]
    for k, v in zip(keys, old):
        _lib.set_tuning(k, v)


def seq_levels(run):
    """rhs, gs(0, 3), residual_norm, restrict(0), gs(1, 1), prolong_add(0) with
    the checker's operators.  The stand-alone residual kernels (norm, restrict)
    evaluate the reference's expressions in both fp modes (csrc/kernels.hip)."""
    O, N, dt, nu, h = run.O, run.N, run.dt, run.nu, 1.0 / run.N
    n1 = N // 2
    out = {}
    run.rhs()
    out["rhs"] = run.t.rhsfine.copy()
    u = run.u
    for _ in range(3):
        O.gauss_seidel(u, run.t.rhsfine, N, run.v1, run.v2, dt, nu, h)
    out["u_gs"] = u.copy()
    O.set_fp_mode(0)
    res = O.residual(u, run.t.rhsfine, N, run.v1, run.v2, dt, nu, h)
    O.set_fp_mode(run.fp)
    out["norm"] = F.Norm(O.compute_norm(res, N), F.accurate_norm(res, N))
    out["rhs1"] = O.restriction(res, N)
    v1c = run.t.level("v1", 1)[: (n1 + 1) ** 2].copy()
    v2c = run.t.level("v2", 1)[: (n1 + 1) ** 2].copy()
    uc = np.zeros((n1 + 1) ** 2)
    O.gauss_seidel(uc, out["rhs1"], n1, v1c, v2c, dt, nu, 2 * h)
    out["u1"] = uc
    out["u_pr"] = u + O.prolongation(uc, n1)
    return out


def interior(a, n):
    return a.reshape(n + 1, n + 1)[1:n, 1:n]


# fp_mode fma changes the temporally blocked smoother (0) only: the other
# smoothers' fma runs would repeat their bitwise ones
LEVEL_CASES = [(s, f, BITWISE) for s, f in SMOOTHERS] + [(s, f, FMA) for s, f in SMOOTHERS if s == 0]


@pytest.mark.parametrize("smoother,fuse,fp", LEVEL_CASES,
                         ids=[f"s{s}f{f}{'fma' if fp else ''}" for s, f, fp in LEVEL_CASES])
@pytest.mark.parametrize("pname", ["easy", "stiff"])
@pytest.mark.parametrize("N", [128, 512])
def test_level_passes_vs_checker(oracle_mod, N, pname, smoother, fuse, fp, tile_mode):
    """Every level op on generic(boundary=True), whole arrays, ring included."""
    L = 3
    want = checker(oracle_mod, seq_levels, "generic", pname, N, L, fp=fp)
    u0, v1, v2 = field("generic", N)
    dt, nu = F.params(pname, N)
    n1 = N // 2
    with Multigrid(N, L, dt, nu, smoother=smoother, fuse=fuse, fp_mode=fp) as mg:
        mg.upload(u0, v1, v2)
        assert mg.velocity_factored() == 0          # the 2-D velocity reads
        mg.rhs()
        assert np.array_equal(interior(mg.download_level(0, "rhs"), N), interior(want["rhs"], N))
        mg.profile(True)
        mg.gs(0, 3)
        assert mg.profile_get(_lib.K_GS, 0)[0] >= 1
        bits_equal(mg.download(), want["u_gs"], N, "u after gs(0, 3)")
        norms_close(mg.residual_norm(0), want["norm"], "residual_norm(0)")
        mg.restrict(0)
        assert np.array_equal(interior(mg.download_level(1, "rhs"), n1),
                              interior(want["rhs1"], n1))
        assert not mg.download_level(1, "u").any()
        mg.gs(1, 1)
        bits_equal(mg.download_level(1, "u"), want["u1"], n1, "u[1] after gs(1, 1)")
        mg.prolong_add(0)
        bits_equal(mg.download(), want["u_pr"], N, "u after prolong_add(0)")


# ---------------------------------------------------------------- b. cycles

def seq_cycles(run):
    """rhs; run_cycles(1) x 2, run_cycles(2); download; mg_outer(TOL_CONTINUED).
    W-cycles: without the run_cycles(2) -- a W-cycle reduces the norm like two
    V-cycles, and after four of them it is at the rounding floor (measured:
    2.6e-9 absolute, where the continued mg_outer stagnates at 1.2e-6 of it)."""
    run.rhs()
    norms = [run.cycle() for _ in range(4 if run.shape == 1 else 2)]
    u4 = run.u.copy()
    cyc, r0, hist = run.mg_outer(TOL_CONTINUED)
    return dict(norms=norms[:2] + norms[3:], u4=u4, cyc=cyc, r0=r0, hist=hist, u=run.u.copy())


def seq_outer(run):
    """rhs; mg_outer(TOL)."""
    run.rhs()
    cyc, r0, hist = run.mg_outer(TOL)
    return dict(cyc=cyc, r0=r0, hist=hist, u=run.u.copy())


def gpu_cycles(mg, N, want, wanto, upload):
    """Both sequences on one solver (the second after a fresh upload); ->
    the finest-level cross pass launches of the whole run."""
    upload(mg)
    mg.rhs()
    mg.profile(True, finest_only=True)
    norms = [mg.run_cycles(1), mg.run_cycles(1)]
    if len(want["norms"]) == 3:
        norms.append(mg.run_cycles(2))
    bits_equal(mg.download(), want["u4"], N, "u after the run_cycles calls")
    norms_close(norms, want["norms"], "run_cycles norms")
    cyc, r0, r, capped = mg.mg_outer(TOL_CONTINUED)
    assert (cyc, capped) == (want["cyc"], False)
    bits_equal(mg.download(), want["u"], N, "u after the continued mg_outer")
    norms_close([r0, r], [want["r0"], want["hist"][-1]], "continued mg_outer norms")
    upload(mg)
    mg.rhs()
    cyc, r0, r, capped = mg.mg_outer(TOL)
    assert (cyc, capped) == (wanto["cyc"], False)
    bits_equal(mg.download(), wanto["u"], N, "u after a fresh mg_outer")
    norms_close([r0, r], [wanto["r0"], wanto["hist"][-1]], "fresh mg_outer norms")
    x = mg.profile_get(_lib.K_XSMOOTH, 0)[0]
    mg.profile(False)
    return x


def cycles_case(O, name, L, tower, fp, nsmooth=3, shape=1, parts=0, device_upload=False,
                expect_cross=True, N=4096):
    want = checker(O, seq_cycles, name, "stiff", N, L, tower, nsmooth, shape, fp)
    wanto = checker(O, seq_outer, name, "stiff", N, L, tower, nsmooth, shape, fp)
    margins_ok((want["r0"], want["hist"], TOL_CONTINUED), (wanto["r0"], wanto["hist"], TOL))
    assert wanto["cyc"] >= 3            # the multi-cycle state is exercised
    u0, v1, v2 = field(name, N)
    if device_upload:
        d = [dev(a) for a in (u0, v1, v2)]
        upload = lambda mg: mg.upload(*d)
    else:
        upload = lambda mg: mg.upload(u0, v1, v2)
    dt, nu = F.params("stiff", N)
    with Multigrid(N, L, dt, nu, nsmooth=nsmooth, shape=shape, tower_mode=tower, fp_mode=fp,
                   local_parts=parts) as mg:
        x = gpu_cycles(mg, N, want, wanto, upload)
        assert (x > 0) == expect_cross, x
        if not parts:
            assert mg.velocity_factored() == 0
        return mg.dist_info() if parts else None


@pytest.mark.parametrize("fp", [BITWISE, FMA], ids=["bitwise", "fma"])
@pytest.mark.parametrize("tower", [REF, CORRECT], ids=["reference", "correct"])
def test_cycles_vs_checker(oracle_mod, tower, fp):
    """N=4096 (the smallest size with the cross-cycle pass), L=5, stiff."""
    cycles_case(oracle_mod, "generic", 5, tower, fp)


@pytest.mark.parametrize("L,fp,kw", [(4, FMA, dict(nsmooth=2)), (4, FMA, dict(shape=2)),
                                     (7, BITWISE, dict(shape=2)), (7, FMA, dict(shape=2))],
                         ids=["nsmooth2", "W", "W-L7-bitwise", "W-L7-fma"])
def test_cycles_vs_checker_other_schedules(oracle_mod, L, fp, kw):
    """L=4: the coarsest level (n = 512) is solved by the host loop.  W-cycles
    at L=7 (tests/schedules.py's N=4096 case): the coarsest n = 64 is solved in
    LDS inside the pair pass of level 5, which restricts into the level's
    second rhs; levels 2-5 run pair passes, level 1 marches, and level 0 takes
    its two visits around the cross pass."""
    cycles_case(oracle_mod, "generic", L, REF, fp, **kw)


def test_cycles_vs_checker_zero_boundary(oracle_mod):
    cycles_case(oracle_mod, "generic0", 5, REF, FMA)


KNOBS = [
    ("cross_cycle0", dict(cross_cycle=0), {}, False),
    ("xfast0", dict(xfast=0), {}, True),
    ("edge_tiles", dict(xtile_max_rows=8193), {}, True),
    ("edge_march", dict(xtile_max_rows=0), {}, True),
    ("zero_rows0", dict(zero_rows=0), {}, True),
    ("post_predict_never", dict(post_predict=-1), {}, True),
    ("post_only_always", dict(post_only=-1), {}, True),
    ("graph_level3", dict(graph_level=3), {}, True),
    ("parts4", {}, dict(parts=4), True),
    ("parts2_replicated", dict(dist_min_rows=8192), dict(parts=2), True),
    ("device_upload", {}, dict(device_upload=True), True),
]


@pytest.mark.parametrize("kv,kw,cross", [k[1:] for k in KNOBS], ids=[k[0] for k in KNOBS])
def test_cycles_knobs_vs_checker(oracle_mod, knobs, kv, kw, cross):
    """The reference-tower / fma case under each knob, against the one checker
    result: the unfused schedule, the guarded cross kernel, the edges of the
    unguarded one as LDS tiles (also the default at this size) and as the
    guarded march, every velocity row read, u_post always recomputed, post-only cycles,
    graph replay, row blocks, replicated parts and a device upload."""
    knobs(**kv)
    for k, v in kv.items():
        assert _lib.get_tuning(k) == v
    g0 = _lib.get_tuning("graph_captures"), _lib.get_tuning("graph_replays")
    info = cycles_case(oracle_mod, "generic", 5, REF, FMA, expect_cross=cross, **kw)
    if "graph_level" in kv:
        assert _lib.get_tuning("graph_captures") > g0[0]
        assert _lib.get_tuning("graph_replays") > g0[1]
    if kw.get("parts") == 4:
        assert info[0] == 4 and info[2] >= 1, info      # level 0 is partitioned
    if kw.get("parts") == 2:
        assert info[0] == 2 and info[2] == 0, info      # everything replicated


# ---------------------------------------------------------------- c. time steps

def seq_steps3(run):
    return _steps(run, 3)


def seq_steps2(run):
    return _steps(run, 2)


def _steps(run, k):
    out = [run.step(TOL) for _ in range(k)]
    return dict(cyc=[o[0] for o in out], r0=[o[1] for o in out], hist=[o[2] for o in out],
                u=run.u.copy())


def steps_case(O, seq, k, name, pname, N, L, tower, fp, parts=0, check_factored=None):
    """-> (dist_info or None, launches at level 0: {K_RHS, K_GS, K_XSMOOTH})."""
    want = checker(O, seq, name, pname, N, L, tower, fp=fp)
    margins_ok(*[(r0, h, TOL) for r0, h in zip(want["r0"], want["hist"])])
    u0, v1, v2 = field(name, N)
    dt, nu = F.params(pname, N)
    with Multigrid(N, L, dt, nu, tower_mode=tower, fp_mode=fp, local_parts=parts) as mg:
        mg.upload(u0, v1, v2)
        if check_factored is not None:
            assert mg.velocity_factored() == check_factored
        mg.profile(True, finest_only=True)
        got = [mg.step_ex(TOL) for _ in range(k)]
        n = {kind: mg.profile_get(kind, 0)[0] for kind in (_lib.K_RHS, _lib.K_GS, _lib.K_XSMOOTH)}
        mg.profile(False)
        assert [g[0] for g in got] == want["cyc"]
        bits_equal(mg.download(), want["u"], N, f"u after {k} steps")
        norms_close([g[1] for g in got], want["r0"], "initial norms of the steps")
        norms_close([g[2] for g in got], [h[-1] for h in want["hist"]], "last norms of the steps")
        assert n[_lib.K_XSMOOTH] > 0, n               # the cross pass ran
        return (mg.dist_info() if parts else None), n


def test_steps_vs_checker_step_fuse(oracle_mod, knobs):
    """Three stiff steps at N=4096, L=5 (multigrid.cpp:165-172, T = 3.5 dt)
    with compute_rhs + initial norm + first pre-smoothing as one pass
    (step_fuse 1, op_rhs_norm_pre) and as an rhs + norm pass followed by the
    first cycle's own pre-smoothing pass (0).  Both run one rhs pass per step;
    the fused schedule runs one finest-level smoothing pass per step fewer --
    were step_fuse ignored, or the fused pass declined, the counts would be
    equal."""
    n = {}
    for step_fuse in (1, 0):
        knobs(step_fuse=step_fuse)
        assert _lib.get_tuning("step_fuse") == step_fuse
        _, n[step_fuse] = steps_case(oracle_mod, seq_steps3, 3, "generic", "stiff", 4096, 5, REF,
                                     FMA, check_factored=0)
    assert n[1][_lib.K_RHS] == n[0][_lib.K_RHS] == 3, n
    assert n[0][_lib.K_GS] - n[1][_lib.K_GS] == 3, n
    assert n[0][_lib.K_XSMOOTH] == n[1][_lib.K_XSMOOTH], n


def test_steps_vs_checker_row_blocks(oracle_mod):
    """The same three steps on four virtual ranks."""
    info, _ = steps_case(oracle_mod, seq_steps3, 3, "generic", "stiff", 4096, 5, REF, FMA, parts=4)
    assert info[0] == 4 and info[2] >= 1, info


@pytest.mark.slow
@pytest.mark.parametrize("step_cross", [1, 0])
def test_steps_N8192_step_cross_vs_checker(oracle_mod, knobs, step_cross):
    """N=8192, L=6, easy, bitwise: the smallest size at which a step's last
    cycle also forms the next step's rhs, norm and pre-smoothing (xstep).
    That it did: one rhs + norm pass over the two steps, the first step's,
    against one per step with step_cross 0 (tests/test_gpu_solver.py counts
    the same) -- every fallback to the plain schedule (no second rhs buffer,
    an unsupported size or kernel variant) launches the second one."""
    knobs(step_cross=step_cross)
    assert _lib.get_tuning("step_cross") == step_cross
    _, n = steps_case(oracle_mod, seq_steps2, 2, "generic", "easy", 8192, 6, REF, BITWISE,
                      check_factored=0)
    assert n[_lib.K_RHS] == (1 if step_cross else 2), n


# ---------------------------------------------------------------- d. rank-1 flow

def seq_rank1(run):
    """rhs; run_cycles(2); download; two steps."""
    run.rhs()
    run.cycle()
    r2 = run.cycle()
    u2 = run.u.copy()
    out = _steps(run, 2)
    out.update(r2=r2, u2=u2)
    return out


def rank1_run(mg, N, want, upload):
    upload(mg)
    mg.rhs()
    mg.profile(True, finest_only=True)
    r2 = mg.run_cycles(2)
    bits_equal(mg.download(), want["u2"], N, "u after run_cycles(2)")
    norms_close(r2, want["r2"], "run_cycles(2) norm")
    got = [mg.step_ex(TOL) for _ in range(2)]
    assert mg.profile_get(_lib.K_XSMOOTH, 0)[0] > 0
    mg.profile(False)
    assert [g[0] for g in got] == want["cyc"]
    norms_close([g[1] for g in got], want["r0"], "initial norms of the steps")
    bits_equal(mg.download(), want["u"], N, "u after two steps")
    norms_close([g[2] for g in got], [h[-1] for h in want["hist"]], "last norms of the steps")


R1_N, R1_L = 4096, 7   # the smallest size with factors and generating levels


def rank1_want(O, tower, fp):
    want = checker(O, seq_rank1, "rank1", "stiff", R1_N, R1_L, tower, fp=fp)
    margins_ok(*[(r0, h, TOL) for r0, h in zip(want["r0"], want["hist"])])
    return want


@pytest.mark.parametrize("vgen,sep", [(1, 1), (0, 1), (1, 0), (0, 0)],
                         ids=["generated", "factors_only", "vgen_without_factors", "arrays"])
@pytest.mark.parametrize("tower", [REF, CORRECT], ids=["reference", "correct"])
def test_rank1_flow_vs_checker(oracle_mod, knobs, tower, vgen, sep):
    """Factors the separable-velocity and generator kernels have never seen
    (zeros, a -0.0, the unit column elsewhere), fma mode: the factor kernels,
    the generated coarse velocity and the 2-D arrays all equal the checker."""
    knobs(vgen=vgen, sep_velocity=sep)
    want = rank1_want(oracle_mod, tower, FMA)
    u0, v1, v2 = field("rank1", R1_N)
    dt, nu = F.params("stiff", R1_N)
    full = 7 if tower == REF else (1 << (R1_L - 1)) - 1
    with Multigrid(R1_N, R1_L, dt, nu, tower_mode=tower, fp_mode=FMA) as mg:
        rank1_run(mg, R1_N, want, lambda m: m.upload(u0, v1, v2))
        assert mg.velocity_factored() == (0 if not sep else full if vgen else 1)


def test_rank1_flow_bitwise_mode_vs_checker(oracle_mod):
    want = rank1_want(oracle_mod, REF, BITWISE)
    u0, v1, v2 = field("rank1", R1_N)
    dt, nu = F.params("stiff", R1_N)
    with Multigrid(R1_N, R1_L, dt, nu) as mg:
        rank1_run(mg, R1_N, want, lambda m: m.upload(u0, v1, v2))
        assert mg.velocity_factored() == 7


@pytest.mark.parametrize("rows", [False, True], ids=["upload", "upload_rows"])
def test_rank1_flow_on_row_blocks_vs_checker(oracle_mod, rows):
    """Two virtual ranks, correct tower: the whole-grid upload and the
    row-block upload (blocks sliced from the same arrays at dist_rows)."""
    want = rank1_want(oracle_mod, CORRECT, FMA)
    u0, v1, v2 = field("rank1", R1_N)
    dt, nu = F.params("stiff", R1_N)
    W = R1_N + 1

    def upload(mg):
        if not rows:
            return mg.upload(u0, v1, v2)
        blocks = []
        for part in range(2):
            lo, hi = mg.dist_rows(part)
            blocks.append(tuple(np.ascontiguousarray(a[lo * W:(hi + 1) * W])
                                for a in (u0, v1, v2)))
        mg.upload_rows(blocks)

    with Multigrid(R1_N, R1_L, dt, nu, tower_mode=CORRECT, fp_mode=FMA, local_parts=2) as mg:
        rank1_run(mg, R1_N, want, upload)
        world, _, la = mg.dist_info()
        assert world == 2 and la >= 2
        fac = mg.velocity_factored()
        assert fac & 1
        if rows:
            assert fac == (1 << la) - 1, (bin(fac), la)

"""Solver-level mirror of the reference's multigrid.cpp on the MI355X path.

* ``init_problem(N)``  -- multigrid.cpp:206-233 (host, glibc libm, bitwise inputs)
* ``timestepper(...)`` -- multigrid.cpp:124-186, same signature; host numpy arrays
* ``Multigrid``        -- the level towers resident in HBM (multigrid.cpp:131-162)
  with ``mg_inner()`` (multigrid.cpp:17-92, one V/W-cycle), ``mg_outer()``
  (multigrid.cpp:97-120), ``step()`` (one timestep, :165-172) and the op-level
  pieces ``gs``, ``residual_norm``, ``restrict``, ``prolong_add``, ``rhs``.

All compute runs in libmgx.so on the GPU; this module only marshals arguments.
"""
from __future__ import annotations

import collections
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, default_options, lib


def _np_ptr(a: np.ndarray):
    if a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"]:
        raise ValueError("expected a C-contiguous float64 array")
    return a.ctypes.data


def default_maxlvl(N: int) -> int:
    """multigrid.cpp:193: int(log2(N)) - 4 (coarsest n = 16... solved by GS)."""
    return int(math.log2(N)) - 4


def init_problem(N: int, nthreads: int = 0):
    """multigrid.cpp:206-233 -> (u0, v1, v2), each (N+1)^2 float64."""
    cnt = (N + 1) * (N + 1)
    u0, v1, v2 = (np.empty(cnt, dtype=np.float64) for _ in range(3))
    check(lib().mgx_init_problem(_np_ptr(u0), _np_ptr(v1), _np_ptr(v2), N, nthreads))
    return u0, v1, v2


def init_problem_rows(N: int, r0: int, r1: int, nthreads: int = 0):
    """Rows [r0, r1) of init_problem(N): three (r1-r0)*(N+1) float64 arrays."""
    cnt = (r1 - r0) * (N + 1)
    u0, v1, v2 = (np.empty(cnt, dtype=np.float64) for _ in range(3))
    check(lib().mgx_init_problem_rows(_np_ptr(u0), _np_ptr(v1), _np_ptr(v2), N, r0, r1,
                                      nthreads))
    return u0, v1, v2


def timestepper(uT, u0, v1, v2, nu, maxlvl, n, dt, T, dx, tol, shape=1, *, nsmooth=3,
                tower_mode=_lib.TOWER_REFERENCE, device=-1, fp_mode=_lib.FP_BITWISE,
                max_cycle=50, coarse_tol=1e-5, coarse_maxit=1000):
    """multigrid.cpp:124 -- run (int)(T/dt) CN steps; writes uT, returns cycles per step.
    A step that ends at max_cycle is not an error (multigrid.cpp:117-119 only
    warns): its entry is max_cycle and the next step starts from its u."""
    steps = int(T / dt)
    cyc = (C.c_int * max(steps, 1))()
    opt = default_options(shape=shape, nsmooth=nsmooth, tower_mode=tower_mode, device=device,
                          fp_mode=fp_mode, max_cycle=max_cycle, coarse_tol=coarse_tol,
                          coarse_maxit=coarse_maxit)
    check(lib().mgx_timestepper_ex(_np_ptr(uT), _np_ptr(u0), _np_ptr(v1), _np_ptr(v2), nu,
                                   maxlvl, n, dt, T, dx, tol, C.byref(opt), cyc))
    return list(cyc)[:steps]


def write_uT(path, rows, N: int, r0: int = 0, r1: int = None, append=False, nthreads=0):
    """multigrid.cpp:269-284 text output ("%d\t%d\t%f\n", i outer, j inner) of
    rows [r0, r1) held in `rows`; rank-ordered appends of row blocks give the
    whole-grid file byte for byte."""
    r1 = N + 1 if r1 is None else r1
    if rows.size != (r1 - r0) * (N + 1):
        raise ValueError("rows must hold (r1-r0)*(N+1) doubles")
    check(lib().mgx_write_uT(str(path).encode(), _np_ptr(rows), N, r0, r1, int(bool(append)),
                             nthreads))


FieldStats = collections.namedtuple(
    "FieldStats", "count nonfinite sum sum_abs sum_sq min max min_i min_j max_i max_j")
FieldStats.__doc__ = "mgx_stats (include/mgx.h) as Multigrid.stats() returns it."


class Multigrid:
    """Device-resident level towers and the V-cycle (mgx_ctx).

    Row-partitioned multi-GPU: ``world > 1`` with ``rank`` and the
    ``unique_id`` from ``dist.unique_id()`` (one process per GPU, RCCL), or
    ``local_parts=G`` for G virtual ranks on this GPU.  A partitioned solver
    takes the whole-solver calls (upload/download of the full grid, rhs,
    mg_inner, mg_outer, step, run_cycles, residual_norm(0)).

    ``capped``: whether the last mg_outer / step / step_ex / step_bdf2 ran its
    ``max_cycle`` cycles (MGX_E_NOCONV; also when the last allowed cycle itself
    reached the tolerance), None before the first of them.
    """

    def __init__(self, N, maxlvl, dt, nu, *, nsmooth=3, shape=1,
                 tower_mode=_lib.TOWER_REFERENCE, device=-1, smoother=0, fuse=3,
                 coarse_tol=1e-5, coarse_maxit=1000, max_cycle=50,
                 world=1, rank=0, unique_id=None, local_parts=0, fp_mode=_lib.FP_BITWISE):
        self.N, self.maxlvl, self.dt, self.nu = N, maxlvl, dt, nu
        self.theta = 0.5   # Crank-Nicolson until set_time_step()
        self.capped = None
        self.opt = default_options(nsmooth=nsmooth, shape=shape, tower_mode=tower_mode,
                                   device=device, smoother=smoother, fuse=fuse,
                                   coarse_tol=coarse_tol,
                                   coarse_maxit=coarse_maxit, max_cycle=max_cycle,
                                   fp_mode=fp_mode)
        h = C.c_void_p()
        if local_parts:
            check(lib().mgx_create_local_dist(C.byref(h), N, maxlvl, dt, nu,
                                              C.byref(self.opt), local_parts))
        elif world > 1 or unique_id is not None:
            if unique_id is None or len(unique_id) != _lib.UNIQUE_ID_BYTES:
                raise ValueError("world > 1 needs the 128-byte unique_id from rank 0")
            idbuf = C.create_string_buffer(bytes(unique_id), _lib.UNIQUE_ID_BYTES)
            check(lib().mgx_create_dist(C.byref(h), N, maxlvl, dt, nu, C.byref(self.opt),
                                        rank, world, idbuf))
        else:
            check(lib().mgx_create(C.byref(h), N, maxlvl, dt, nu, C.byref(self.opt)))
        self._h = h

    def dist_info(self):
        """-> (world, rank, first replicated level); rank -1 for local parts."""
        w, r, la = C.c_int(), C.c_int(), C.c_int()
        check(lib().mgx_dist_info(self._h, C.byref(w), C.byref(r), C.byref(la)))
        return w.value, r.value, la.value

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().mgx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # -- data
    def upload(self, u0, v1, v2):
        if isinstance(u0, np.ndarray):
            check(lib().mgx_upload(self._h, _np_ptr(u0), _np_ptr(v1), _np_ptr(v2)))
        else:   # device tensors in the reference layout
            check(lib().mgx_upload_device(self._h, u0.data_ptr(), v1.data_ptr(),
                                          v2.data_ptr()))

    def set_velocity(self, v1, v2):
        """Replace the velocity and keep the finest-level u (mgx_set_velocity):
        the same, bit for bit, as download() + upload(u, v1, v2) without moving
        u.  numpy arrays or device tensors in the reference layout; call rhs()
        or step() next.  Single-GPU solvers only."""
        if isinstance(v1, np.ndarray):
            check(lib().mgx_set_velocity(self._h, _np_ptr(v1), _np_ptr(v2)))
        else:
            check(lib().mgx_set_velocity_device(self._h, v1.data_ptr(), v2.data_ptr()))

    def set_source(self, f):
        """Source term of u_t + v.grad u = nu lap u + f (mgx_set_source): every
        rhs() and step() from now on adds fl(fl(dt * scale) * f) to the
        interior of the right-hand side.  f: a numpy array or a device tensor
        in the reference layout ((N+1)^2 float64; the solver keeps its own
        copy), or None to remove the source.  Survives upload() and
        set_velocity(); call rhs() or step() next."""
        if f is None:
            check(lib().mgx_set_source(self._h, None))
        elif isinstance(f, np.ndarray):
            if f.size != (self.N + 1) ** 2:
                raise ValueError("f must hold (N+1)^2 doubles")
            check(lib().mgx_set_source(self._h, _np_ptr(f)))
        else:
            if f.numel() != (self.N + 1) ** 2 or f.element_size() != 8 or not f.is_contiguous():
                raise ValueError("f must be a contiguous float64 tensor of (N+1)^2 entries")
            check(lib().mgx_set_source_device(self._h, f.data_ptr()))

    def set_source_separable(self, a, b):
        """A source given by its factors (mgx_set_source_separable): f(i,j) =
        a[0][i]*b[0][j] (+ a[1][i]*b[1][j] ...), each product rounded and the
        terms added left to right -- bit for bit set_source() of that array,
        with no finest-level array kept and no source stream read.  a (rows)
        and b (columns): 1-D arrays of N+1 for one term or (R, N+1) arrays, R
        <= 4; numpy arrays, or torch tensors on the solver's device.  Replaces
        a source of either kind; calling it again replaces the factors in
        place (a moving emitter: one call per step).  Every kind of solver
        takes it; RCCL ranks must all pass the same values."""
        host = isinstance(a, np.ndarray)
        if host != isinstance(b, np.ndarray):
            raise ValueError("a and b must both be numpy arrays or both device tensors")
        sa, sb = tuple(a.shape), tuple(b.shape)
        if sa != sb or len(sa) not in (1, 2) or sa[-1] != self.N + 1:
            raise ValueError("a and b must both have shape (N+1,) or (R, N+1)")
        terms = 1 if len(sa) == 1 else sa[0]
        if not 1 <= terms <= _lib.MGX_SOURCE_MAX_TERMS:
            raise ValueError(f"a separable source has 1..{_lib.MGX_SOURCE_MAX_TERMS} terms")
        if host:
            check(lib().mgx_set_source_separable(self._h, terms, _np_ptr(a), _np_ptr(b)))
        else:
            for x in (a, b):
                if x.element_size() != 8 or not x.is_contiguous():
                    raise ValueError("a, b must be contiguous float64 tensors")
            check(lib().mgx_set_source_separable_device(self._h, terms, a.data_ptr(),
                                                        b.data_ptr()))

    def set_source_rows(self, blocks):
        """Row-block set_source (mgx_set_source_rows) for solvers on which
        nobody holds the whole grid: blocks[i] = the source on the OWNED rows
        [ra, rb) (owned_rows) of local part i, (rb-ra)*(N+1) float64, all numpy
        arrays or all device tensors.  Needs a partitioned level (dist_info);
        on a single-GPU solver the one block is the whole grid."""
        blocks = list(blocks)
        host = all(isinstance(x, np.ndarray) for x in blocks)
        if not host and any(isinstance(x, np.ndarray) for x in blocks):
            raise ValueError("blocks must all be numpy arrays or all device tensors")
        world, rank, _ = self.dist_info()
        parts = world if rank < 0 else 1
        if len(blocks) != parts:
            raise ValueError(f"expected {parts} blocks, one per local part")
        ptrs = []
        for i, x in enumerate(blocks):
            ra, rb = self.owned_rows(i)
            cnt = (rb - ra) * (self.N + 1)
            if host:
                if x.size != cnt:
                    raise ValueError(f"block {i} must hold {cnt} doubles")
                ptrs.append(_np_ptr(x))
            else:
                if x.numel() != cnt or x.element_size() != 8 or not x.is_contiguous():
                    raise ValueError(f"block {i} must be a contiguous float64 tensor of {cnt} "
                                     "entries")
                ptrs.append(x.data_ptr())
        arr =(C.c_void_p * len(ptrs))(*ptrs)
        f = lib().mgx_set_source_rows if host else lib().mgx_set_source_rows_device
        check(f(self._h, arr))

    def source_kind(self):
        """-> (kind, terms) (mgx_source_kind): kind 0 none, 1 field (whole grid
        or row blocks), 2 separable; terms: R of a separable source, else 0."""
        k, t = C.c_int(), C.c_int()
        check(lib().mgx_source_kind(self._h, C.byref(k), C.byref(t)))
        return k.value, t.value

    def set_source_scale(self, s):
        """The factor s of the source term fl(dt * s) * f (default 1): a
        time-separable source g(t) f(x, y) needs no new upload per step."""
        check(lib().mgx_set_source_scale(self._h, float(s)))

    def source_info(self):
        """-> (active, scale) (mgx_source_info)."""
        a, s = C.c_int(), C.c_double()
        check(lib().mgx_source_info(self._h, C.byref(a), C.byref(s)))
        return bool(a.value), s.value

    # -- time-dependent Dirichlet data (mgx_set_boundary)
    _WHEN = {"now": _lib.BC_NOW, "next": _lib.BC_NEXT_STEP}

    def set_boundary(self, g, when="now"):
        """Replace the Dirichlet ring of the finest u (mgx_set_boundary).  g:
        4(N+1) float64, flat or (4, N+1) -- u(0,:), u(N,:), u(:,0), u(:,N); the
        corners are the rows' (entries 0 and N of the two column sides are
        ignored) -- a numpy array or a torch tensor on the solver's device.
        when="now": the ring is overwritten at once, every other bit of u and
        the right-hand side stay.  when="next": the solver keeps a copy and the
        next step() / step_ex() is rhs(); set_boundary(g, "now"); mg_outer()
        bit for bit -- the Crank-Nicolson step from the old ring to the new
        one; g=None cancels it.  Every kind of solver takes it; RCCL ranks
        must all pass the same values."""
        if when not in self._WHEN:
            raise _lib.MGXError(_lib.MGX_E_ARG, "set_boundary: when must be 'now' or 'next'")
        w = self._WHEN[when]
        cnt = 4 * (self.N + 1)
        if g is None:
            check(lib().mgx_set_boundary(self._h, None, w))
        elif isinstance(g, np.ndarray):
            if g.size != cnt:
                raise ValueError(f"g must hold {cnt} doubles")
            check(lib().mgx_set_boundary(self._h, _np_ptr(g), w))
        else:
            if g.numel() != cnt:
                raise ValueError(f"g must hold {cnt} doubles")
            check(lib().mgx_set_boundary_device(self._h, _lib.device_ptr(g, cnt, "g"), w))

    def get_boundary(self, out=None):
        """The ring of the finest u (mgx_get_boundary) -> a (4, N+1) array, the
        corner entries of the column sides filled with the corner values.  out:
        a numpy array, or a device tensor the kernel writes directly.
        Single-GPU and local-parts solvers."""
        cnt = 4 * (self.N + 1)
        if out is not None and not isinstance(out, np.ndarray):
            check(lib().mgx_get_boundary_device(self._h, _lib.device_ptr(out, cnt, "out")))
            return out
        out = np.empty((4, self.N + 1), dtype=np.float64) if out is None else out
        if out.size != cnt:
            raise ValueError(f"out must hold {cnt} doubles")
        check(lib().mgx_get_boundary(self._h, _np_ptr(out)))
        return out

    def boundary_pending(self):
        """1 while a ring set with when="next" waits for the next step, else 0
        (mgx_boundary_info)."""
        p = C.c_int()
        check(lib().mgx_boundary_info(self._h, C.byref(p)))
        return p.value

    # -- per-step dt and theta (mgx_set_time_step)
    def set_time_step(self, dt=None, theta=None):
        """The time step and the scheme of every later step (mgx_set_time_step):
        (I + theta dt L) u' = (I - (1 - theta) dt L) u + dt f.  None keeps the
        current value.  theta=0.5 is Crank-Nicolson (the solver's schedule as
        before, bit for bit with the dt of the constructor), theta=1 implicit
        Euler.  u, the right-hand side, the velocity, a source and a pending
        ring stay; what was formed with the old coefficients is dropped.
        self.dt and self.theta follow, so cfl() reports the new number.  RCCL
        ranks must all pass the same values."""
        cur_dt, cur_theta = self.time_step()
        dt = cur_dt if dt is None else float(dt)
        theta = cur_theta if theta is None else float(theta)
        check(lib().mgx_set_time_step(self._h, dt, theta))
        self.dt, self.theta = dt, theta

    def time_step(self):
        """-> (dt, theta) (mgx_time_step_info)."""
        dt, th = C.c_double(), C.c_double()
        check(lib().mgx_time_step_info(self._h, C.byref(dt), C.byref(th)))
        return dt.value, th.value

    # -- variable-step BDF2 on a device-resident history (mgx_set_history)
    def set_history(self, on=True):
        """mgx_set_history: keep one more finest-level array h on the device
        (one per part) that holds u^n while u becomes u^(n+1) -- what
        step_bdf2() and rollback() need.  Every step() / step_ex() / step_bdf2()
        then begins by making h what download() would return.  on=False frees
        it.  Raises MGXError (MGX_E_HIP) where there is no room."""
        check(lib().mgx_set_history(self._h, 1 if on else 0))

    def history_info(self):
        """-> dict(on, valid, dt_prev, k_solve) (mgx_history_info): valid = h
        holds the u the last step started from, dt_prev = that step's dt,
        k_solve = the k every solve-side call currently uses."""
        on, valid = C.c_int(), C.c_int()
        dtp, ks = C.c_double(), C.c_double()
        check(lib().mgx_history_info(self._h, C.byref(on), C.byref(valid), C.byref(dtp),
                                     C.byref(ks)))
        return {"on": on.value, "valid": valid.value, "dt_prev": dtp.value,
                "k_solve": ks.value}

    def step_bdf2(self, tol=1e-6):
        """One variable-step BDF2 step with the context's dt after the last
        step's (mgx_step_bdf2) -> (cycles, res0, res).  Needs a valid history: a
        theta-step (step()) starts it.  Zero-stability needs dt / dt_prev < 1 +
        sqrt(2); nothing is refused."""
        cyc, r0, r = C.c_int(), C.c_double(), C.c_double()
        rc = check(lib().mgx_step_bdf2(self._h, tol, C.byref(cyc), C.byref(r0), C.byref(r)),
                   allow=(_lib.MGX_E_NOCONV,))
        self.capped = rc == _lib.MGX_E_NOCONV
        return cyc.value, r0.value, r.value

    def rollback(self):
        """mgx_rollback: u becomes the u the last step started from (ring
        included) and the history loses its validity -- the next step is a
        theta-step: call step() next."""
        check(lib().mgx_rollback(self._h))

    # -- a predicted start for BDF2 steps (mgx_set_predictor)
    def set_predictor(self, order):
        """mgx_set_predictor: 0 = off (the default), 1 / 2 = step_bdf2 forms a
        linear / quadratic guess of u^(n+1) from the resident history and
        starts from it where its residual is smaller than u^n's; the stopping
        criterion stays relative to u^n's residual.  Order 2 needs depth 2 and
        two steps of history and falls back to order 1 by itself.  A step that
        takes a pending ring runs unpredicted.  Single-GPU contexts only: a
        partitioned context raises MGXError (MGX_E_ARG) for an order > 0."""
        check(lib().mgx_set_predictor(self._h, int(order)))

    def predictor_info(self):
        """-> dict(order, last_order, adopted, res_pred) (mgx_predictor_info):
        the setting; the effective order of the last step_bdf2 (0: it ran
        unpredicted); whether that step started from the guess; the guess's
        residual norm (0.0 where last_order is 0)."""
        o, lo, ad, rp = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        check(lib().mgx_predictor_info(self._h, C.byref(o), C.byref(lo), C.byref(ad),
                                       C.byref(rp)))
        return {"order": o.value, "last_order": lo.value, "adopted": ad.value,
                "res_pred": rp.value}

    # -- the step error estimate on a two-deep history (mgx_set_history_depth)
    def set_history_depth(self, depth):
        """mgx_set_history_depth: 0 = no history, 1 = set_history(), 2 = a
        second array h2 beside h, so that after a step u^(n+1), u^n and u^(n-1)
        are resident together -- what step_error() needs, and what lets
        rollback() keep u^(n-1) for a BDF2 retry.  No data is copied for it.
        Raises MGXError (MGX_E_HIP) where there is no room; the context then
        keeps the depth it had."""
        check(lib().mgx_set_history_depth(self._h, int(depth)))

    def history_depth(self):
        """-> dict(depth, valid2, dt_prev2) (mgx_history_depth): valid2 = h2
        holds u^(n-1), dt_prev2 = the dt of the step that started from it."""
        d, v2, dt2 = C.c_int(), C.c_int(), C.c_double()
        check(lib().mgx_history_depth(self._h, C.byref(d), C.byref(v2), C.byref(dt2)))
        return {"depth": d.value, "valid2": v2.value, "dt_prev2": dt2.value}

    def step_error(self, atol, rtol):
        """One reduction pass over u, h and h2 after a step (mgx_step_error) ->
        StepError: with w = dt_prev / dt_prev2, at every interior point d = u -
        ((1 + w) h - w h2), c = u - h and e = d / (atol + rtol max(|u|, |h|));
        the sums of squares and the maxima of |e|, |d|, |c| over the points
        with a finite e, where |e| is largest, and .rms of e.  Needs depth 2
        and two steps since the last upload or rollback.  A local-parts solver
        returns the parts' records merged in part order; an RCCL rank calls
        step_error_rows and merges (step_err_merge)."""
        s = _lib.StepErr()
        check(lib().mgx_step_error(self._h, float(atol), float(rtol), C.byref(s)))
        return _lib.StepError(s)

    def step_error_rows(self, part, atol, rtol):
        """step_error() of the owned finest-level rows of local part `part`,
        with global positions and no communication (mgx_step_error_rows)."""
        s = _lib.StepErr()
        check(lib().mgx_step_error_rows(self._h, int(part), float(atol), float(rtol),
                                        C.byref(s)))
        return _lib.StepError(s)

    def velocity_factored(self):
        """mgx_velocity_factored: bit 0 = the finest level keeps velocity
        factors, bit l = level l generates its velocity from them."""
        f = C.c_int(0)
        check(lib().mgx_velocity_factored(self._h, C.byref(f)))
        return f.value

    def dist_rows(self, part=0):
        """-> (lo, hi): allocated finest-level rows of local part `part`."""
        lo, hi = C.c_int(), C.c_int()
        check(lib().mgx_dist_rows(self._h, part, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def upload_rows(self, blocks):
        """Row-block upload: blocks[i] = (u0, v1, v2) rows [lo, hi] of local part i
        (init_problem_rows); needs tower_mode=TOWER_CORRECT."""
        k = len(blocks)
        arr = C.c_void_p * k
        u, a, b = (arr(*[_np_ptr(blk[j]) for blk in blocks]) for j in range(3))
        check(lib().mgx_upload_rows(self._h, u, a, b))

    def owned_rows(self, part=0):
        """-> (ra, rb): finest-level rows [ra, rb) owned by local part `part`."""
        ra, rb = C.c_int(), C.c_int()
        check(lib().mgx_owned_rows(self._h, part, C.byref(ra), C.byref(rb)))
        return ra.value, rb.value

    def download_rows(self, part=0, out=None):
        """Row-block download: the owned rows of local part `part`,
        (rb-ra)*(N+1) float64 (no rank ever holds the whole grid)."""
        ra, rb = self.owned_rows(part)
        cnt = (rb - ra) * (self.N + 1)
        out = np.empty(cnt, dtype=np.float64) if out is None else out
        if out.size != cnt:
            raise ValueError(f"out must hold {cnt} doubles")
        check(lib().mgx_download_rows(self._h, part, _np_ptr(out)))
        return out

    def download(self, out=None):
        out = np.empty((self.N + 1) ** 2, dtype=np.float64) if out is None else out
        check(lib().mgx_download(self._h, _np_ptr(out)))
        return out

    def level_n(self, level):
        n = C.c_long()
        check(lib().mgx_level_n(self._h, level, C.byref(n)))
        return n.value

    def download_level(self, level, field="u"):
        f = {"u": 0, "rhs": 1, "v1": 2, "v2": 3}[field]
        n = self.level_n(level)
        out = np.empty((n + 1) ** 2, dtype=np.float64)
        check(lib().mgx_download_level(self._h, level, f, _np_ptr(out)))
        return out

    # -- field diagnostics on the device (mgx_field_stats, mgx_sample)
    # ("history" / "history2": h and h2 of set_history / set_history_depth, level
    # 0, while they hold a time level)
    _FIELDS = {"u": 0, "rhs": 1, "v1": 2, "v2": 3, "source": 4, "history": 5, "history2": 6}

    def stats(self, field="u", level=0, interior=False, minus=None):
        """One reduction pass over what download_level(level, field) would
        return -> FieldStats (count, nonfinite, sum, sum_abs, sum_sq, min, max,
        min_i, min_j, max_i, max_j; sums and extrema over the finite entries,
        positions of the first occurrence in row-major order).  field: "u",
        "rhs", "v1", "v2" or "source"; interior: rows and columns 1..n-1 only;
        minus: a device tensor in the reference layout of that level -- the
        statistics are then those of fl(field - minus).  A local-parts solver
        takes level 0 (the parts' records merged in part order)."""
        n = self.N if level == 0 else self.level_n(level)
        s = _lib.Stats()
        check(lib().mgx_field_stats(self._h, level, self._FIELDS[field], int(bool(interior)),
                                    _lib.device_ptr(minus, (n + 1) ** 2, "minus"), C.byref(s)))
        return FieldStats(*s.astuple())

    def stats_rows(self, part=0, field="u", interior=False, minus=None):
        """stats() of the owned finest-level rows [ra, rb) of local part `part`
        (owned_rows), with global positions and no communication: what a rank
        of a multi-process run calls, combining the ranks' records with
        stats_merge.  minus: a device tensor of those rows, (rb-ra)*(N+1)."""
        cnt = 0
        if minus is not None:
            ra, rb = self.owned_rows(part)
            cnt = (rb - ra) * (self.N + 1)
        s = _lib.Stats()
        check(lib().mgx_field_stats_rows(self._h, part, self._FIELDS[field], int(bool(interior)),
                                         _lib.device_ptr(minus, cnt, "minus"), C.byref(s)))
        return FieldStats(*s.astuple())

    def sample(self, stride, field="u", level=0, out=None):
        """Every stride-th row and column of a field, gathered on the device:
        bitwise download_level(level, field).reshape(n+1, n+1)[::stride,
        ::stride] -> an (m+1, m+1) array, m = n/stride (stride must divide n).
        out: a numpy array, or a device tensor the kernel writes directly."""
        n = self.N if level == 0 else self.level_n(level)
        if stride < 1 or n % stride:
            raise _lib.MGXError(_lib.MGX_E_ARG, "sample: stride must divide the level's n")
        m = n // stride
        f = self._FIELDS[field]
        if out is not None and not isinstance(out, np.ndarray):
            check(lib().mgx_sample_device(self._h, level, f, stride,
                                          _lib.device_ptr(out, (m + 1) ** 2, "out")))
            return out
        out = np.empty((m + 1, m + 1), dtype=np.float64) if out is None else out
        if out.size != (m + 1) ** 2:
            raise ValueError(f"out must hold {(m + 1) ** 2} doubles")
        check(lib().mgx_sample(self._h, level, f, stride, _np_ptr(out)))
        return out

    def sample_rows(self, part, stride, field="u"):
        """-> (first_row, array): the sampled rows i (i % stride == 0) among
        the owned rows of local part `part`, rows x (N/stride+1); first_row is
        the fine-grid index of the first of them."""
        f = self._FIELDS[field]
        first, rows = C.c_long(), C.c_long()
        check(lib().mgx_sample_rows(self._h, part, f, stride, None, C.byref(first),
                                    C.byref(rows)))
        out = np.empty((rows.value, self.N // stride + 1), dtype=np.float64)
        if rows.value:
            check(lib().mgx_sample_rows(self._h, part, f, stride, _np_ptr(out), C.byref(first),
                                        C.byref(rows)))
        return first.value, out

    # -- dense output (mgx_dense_output, mgx_dense_points)
    def dense(self, order, tau, stride=1, out=None):
        """The interpolant through the resident time levels at tau = t* -
        t^(n+1) <= 0, every stride-th row and column -> an (m+1, m+1) array, m =
        N/stride (mgx_dense_output): order 0 = u, 1 = linear through u and the
        history h, 2 = the quadratic through u, h and h2 (depth 2, two steps),
        with the weights dense_weights(order, tau, dt_prev, dt_prev2).  stride 1
        is the whole field.  out: a numpy array, or a device tensor the kernel
        writes directly.  An RCCL rank calls dense_rows."""
        if stride < 1 or self.N % stride:
            raise _lib.MGXError(_lib.MGX_E_ARG, "dense: stride must divide N")
        m = self.N // stride
        if out is not None and not isinstance(out, np.ndarray):
            check(lib().mgx_dense_output_device(self._h, int(order), float(tau), stride,
                                                _lib.device_ptr(out, (m + 1) ** 2, "out")))
            return out
        out = np.empty((m + 1, m + 1), dtype=np.float64) if out is None else out
        if out.size != (m + 1) ** 2:
            raise ValueError(f"out must hold {(m + 1) ** 2} doubles")
        check(lib().mgx_dense_output(self._h, int(order), float(tau), stride, _np_ptr(out)))
        return out

    def dense_rows(self, part, order, tau, stride=1):
        """-> (first_row, array): dense() of the sampled rows i (i % stride ==
        0) among the owned rows of local part `part`, rows x (N/stride+1), with
        no communication (mgx_dense_output_rows)."""
        first, rows = C.c_long(), C.c_long()
        args = (self._h, int(part), int(order), float(tau), stride)
        check(lib().mgx_dense_output_rows(*args, None, C.byref(first), C.byref(rows)))
        out = np.empty((rows.value, self.N // stride + 1), dtype=np.float64)
        if rows.value:
            check(lib().mgx_dense_output_rows(*args, _np_ptr(out), C.byref(first),
                                              C.byref(rows)))
        return first.value, out

    def dense_points(self, order, tau, i, j, out=None):
        """The interpolant at the grid points (i[k], j[k]) -> one value each
        (probes).  i, j: integer sequences or numpy arrays (mgx_dense_points: a
        bad index raises and names k), or int64 device tensors, with a float64
        device tensor out or a new one (mgx_dense_points_device: a bad index
        gives NaN there)."""
        if not isinstance(i, (np.ndarray, list, tuple)):
            import torch
            if i.dtype != torch.int64 or j.dtype != torch.int64 or i.numel() != j.numel() \
                    or not i.is_contiguous() or not j.is_contiguous():
                raise ValueError("i, j: contiguous int64 device tensors of one length")
            npts = i.numel()
            out = torch.empty(npts, dtype=torch.float64, device=i.device) if out is None else out
            check(lib().mgx_dense_points_device(self._h, int(order), float(tau), npts,
                                                i.data_ptr(), j.data_ptr(),
                                                _lib.device_ptr(out, npts, "out")))
            return out
        pi = np.ascontiguousarray(i, dtype=np.int64)
        pj = np.ascontiguousarray(j, dtype=np.int64)
        if pi.shape != pj.shape or pi.ndim != 1:
            raise ValueError("i, j: one-dimensional index arrays of one length")
        out = np.empty(pi.size, dtype=np.float64) if out is None else out
        if out.size != pi.size:
            raise ValueError(f"out must hold {pi.size} doubles")
        check(lib().mgx_dense_points(self._h, int(order), float(tau), pi.size,
                                     pi.ctypes.data, pj.ctypes.data, _np_ptr(out)))
        return out

    def cfl(self):
        """The CFL number max(max|v1|, max|v2|) * dt * N of the finest level's
        velocity, from two stats() passes (multiplied in that order)."""
        vmax = 0.0
        for f in ("v1", "v2"):
            s = self.stats(f)
            vmax = max(vmax, abs(s.min), abs(s.max)) if s.count > s.nonfinite else vmax
        return vmax * self.dt * self.N

    # -- ops (multigrid.cpp call sites)
    def rhs(self):
        check(lib().mgx_rhs(self._h))

    def gs(self, level, sweeps=1):
        check(lib().mgx_gs(self._h, level, sweeps))

    def residual_norm(self, level=0):
        r = C.c_double()
        check(lib().mgx_residual_norm(self._h, level, C.byref(r)))
        return r.value

    def restrict(self, level):
        check(lib().mgx_restrict(self._h, level))

    def prolong_add(self, level):
        check(lib().mgx_prolong_add(self._h, level))

    def mg_inner(self):
        """multigrid.cpp:17 at lvl=0: one V (shape=1) or W (shape=2) cycle."""
        check(lib().mgx_vcycle(self._h))

    vcycle = mg_inner

    def mg_outer(self, tol=1e-6):
        """multigrid.cpp:97 -> (cycles, res0, res); cap hit is reported, not raised."""
        cyc, r0, r = C.c_int(), C.c_double(), C.c_double()
        rc = check(lib().mgx_mg_outer(self._h, tol, C.byref(cyc), C.byref(r0), C.byref(r)),
                   allow=(_lib.MGX_E_NOCONV,))
        self.capped = rc == _lib.MGX_E_NOCONV
        return cyc.value, r0.value, r.value, self.capped

    def step(self, tol=1e-6):
        """One time step -> cycles; a cap hit is reported in self.capped."""
        cyc = C.c_int()
        rc = check(lib().mgx_step(self._h, tol, C.byref(cyc)), allow=(_lib.MGX_E_NOCONV,))
        self.capped = rc == _lib.MGX_E_NOCONV
        return cyc.value

    def step_ex(self, tol=1e-6):
        """step() -> (cycles, res0, res): with mg_outer's initial and last
        residual norm (mgx_step_ex)."""
        cyc, r0, r = C.c_int(), C.c_double(), C.c_double()
        rc = check(lib().mgx_step_ex(self._h, tol, C.byref(cyc), C.byref(r0), C.byref(r)),
                   allow=(_lib.MGX_E_NOCONV,))
        self.capped = rc == _lib.MGX_E_NOCONV
        return cyc.value, r0.value, r.value

    def run_cycles(self, cycles):
        r = C.c_double()
        check(lib().mgx_run_cycles(self._h, cycles, C.byref(r)))
        return r.value

    def coarse_iterations(self):
        it = C.c_long()
        check(lib().mgx_coarse_iterations(self._h, C.byref(it)))
        return it.value

    def synchronize(self):
        check(lib().mgx_synchronize(self._h))

    def stream(self):
        s = C.c_void_p()
        check(lib().mgx_stream(self._h, C.byref(s)))
        return s.value

    # -- profiling (HIP events on the context stream)
    def profile(self, on=True, finest_only=False):
        """HIP events around launches: all levels, or the finest level only."""
        check(lib().mgx_profile_enable(self._h, (2 if finest_only else 1) if on else 0))

    def profile_reset(self):
        check(lib().mgx_profile_reset(self._h))

    def profile_get(self, kind, level=-1):
        n, ms, b = C.c_long(), C.c_double(), C.c_double()
        check(lib().mgx_profile_get(self._h, kind, level, C.byref(n), C.byref(ms), C.byref(b)))
        return n.value, ms.value, b.value

    def profile_get_ex(self, kind, level=-1):
        """(launches, device ms, canonical algorithmic bytes, compulsory bytes)"""
        n, ms, b, cb = C.c_long(), C.c_double(), C.c_double(), C.c_double()
        check(lib().mgx_profile_get_ex(self._h, kind, level, C.byref(n), C.byref(ms),
                                       C.byref(b), C.byref(cb)))
        return n.value, ms.value, b.value, cb.value

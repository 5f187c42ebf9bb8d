/* mgx.h -- C ABI of the MI355X-native geometric-multigrid V-cycle (libmgx.so).
 *
 * Drop-in boundary for the reference's hot path (soniareilly/HPCClassMultigridProject):
 *   - the op-level seam gs.h:3-17 (gauss_seidel, residual, compute_norm,
 *     prolongation, restriction, compute_rhs), here on DEVICE pointers in the
 *     reference layout (row-major (n+1)^2 doubles, element (i,j) at i*(n+1)+j);
 *   - the solver-level functions multigrid.cpp:17 (mg_inner), :97 (mg_outer)
 *     and :124 (timestepper), here on a context that keeps the level towers
 *     resident in HBM (mgx_ctx), plus mgx_timestepper with the exact reference
 *     signature on HOST arrays.
 *
 * Conventions:
 *   - every function returns 0 on success and a non-zero MGX_E* code on
 *     failure; mgx_last_error() returns the message of the last failure on the
 *     calling thread;
 *   - the caller owns every buffer passed in; ops never allocate;
 *   - raw-pointer ops run on the HIP null stream and are ordered with other
 *     null-stream work; mgx_compute_norm synchronises (it returns a host value,
 *     like gs.cpp:86).  Context functions run on the context's own stream;
 *   - all arithmetic is fp64 with the reference's term order and no FMA
 *     contraction, so op results are bitwise equal to the serial reference
 *     (a context may opt into contracted smoothing passes: MGX_FP_FMA).
 */
#ifndef MGX_H
#define MGX_H

#ifdef __cplusplus
extern "C" {
#endif

#define MGX_OK 0
#define MGX_E_ARG 1     /* invalid argument (sizes, level, null pointer) */
#define MGX_E_HIP 2     /* a HIP runtime call failed */
#define MGX_E_RCCL 3    /* an RCCL call failed */
#define MGX_E_NOCONV 4  /* mg_outer ran max_cycle cycles (reported, not fatal; also
                           when the last of them reached the tolerance) */
#define MGX_E_INTERNAL 5 /* an internal consistency check failed (a bug) */

const char *mgx_last_error(void);
int mgx_version(void);

/* ---------------------------------------------------------------------------
 * Op-level seam: replaces gs.h (reference gs.h:3-17, implementations gs.cpp).
 * Device pointers, reference layout.  k = dt, h = grid spacing at this level.
 * ------------------------------------------------------------------------- */

/* gs.h:9 / gs.cpp:109-189: one red-black Gauss-Seidel sweep, in place. */
int mgx_gauss_seidel(double *u, const double *rhs, long n, const double *v1,
                     const double *v2, double k, double nu, double h);
/* gs.h:3 / gs.cpp:55-83: res = rhs - A u on the interior; res boundary untouched. */
int mgx_residual(double *res, const double *u, const double *rhs, long n,
                 const double *v1, const double *v2, double k, double nu, double h);
/* gs.h:5 / gs.cpp:86-107: *norm = sqrt(sum of interior res^2).  Does not modify res. */
int mgx_compute_norm(const double *res, long n, double *norm);
/* gs.h:16 / gs.cpp:228-266: bilinear prolongation, up (2n+1)^2 <- u (n+1)^2. */
int mgx_prolongation(double *up, const double *u, long n);
/* gs.h:17 / gs.cpp:268-292: injection, u (n/2+1)^2 <- up (n+1)^2 (incl. boundary). */
int mgx_restriction(double *u, const double *up, long n);
/* gs.h:13 / gs.cpp:24-53: Crank-Nicolson right-hand side B u on the interior. */
int mgx_compute_rhs(double *rhs, const double *u, long n, const double *v1,
                    const double *v2, double k, double nu, double h);

/* multigrid.cpp:206-233: the reference problem on the host with the C library
 * (glibc) exp/sin/cos, so inputs are bitwise those of the reference: Gaussian
 * u0 (x0=.2, y0=.4, sigma=100) with zero boundary, v1 = -pi sin(pi x) cos(pi y),
 * v2 = pi cos(pi x) sin(pi y); x = i/N, y = j/N.  Arrays of (N+1)^2 doubles.
 * nthreads <= 0: all hardware threads. */
int mgx_init_problem(double *u0, double *v1, double *v2, long N, int nthreads);
/* Rows [r0, r1) only, into arrays of (r1-r0)*(N+1) doubles: bitwise those rows
 * of mgx_init_problem (for row-block uploads, mgx_upload_rows). */
int mgx_init_problem_rows(double *u0, double *v1, double *v2, long N, long r0, long r1,
                          int nthreads);

/* ---------------------------------------------------------------------------
 * Solver level.
 * ------------------------------------------------------------------------- */

/* Tower construction (multigrid.cpp:148-160). */
#define MGX_TOWER_REFERENCE 0 /* bitwise reference semantics (index quirk, zero fill) */
#define MGX_TOWER_CORRECT 1   /* every level injected from the level above */

typedef struct mgx_options {
    int nsmooth;        /* RB-GS sweeps before and after the coarse correction
                           (NITER, multigrid.cpp:41; reference 3) */
    int shape;          /* 1 = V-cycle, 2 = W-cycle (multigrid.cpp:52) */
    int tower_mode;     /* MGX_TOWER_* (default REFERENCE) */
    int device;         /* HIP device ordinal for this context */
    double coarse_tol;  /* coarsest-level GS stop, absolute (multigrid.cpp:60: 1e-5) */
    int coarse_maxit;   /* coarsest-level GS cap (multigrid.cpp:60: 1000) */
    int max_cycle;      /* mg_outer cycle cap (multigrid.cpp:94: 50) */
    int smoother;       /* 0 = temporally blocked passes of up to `fuse` sweeps with
                           the prolongation fused into the post-smoothing pass
                           (default); 1 = two in-place colour passes per sweep;
                           2 = one-pass single sweeps (no temporal blocking) */
    int fuse;           /* smoother 0: max RB sweeps per HBM pass, 1..3 (default 3) */
    int fp_mode;        /* MGX_FP_BITWISE (default) or MGX_FP_FMA, below */
} mgx_options;

/* Arithmetic of the smoothing passes (smoother 0: the fused row marches,
 * LDS tiles and the coarsest solve; the gs.h mirror ops, smoothers 1/2 and
 * compute_rhs are always bitwise).
 * MGX_FP_BITWISE: the reference's expressions term by term, no contraction,
 *   the correctly rounded division -- u bitwise equal to the serial reference.
 *   Domain: finite fields whose update numerators a = rhs - sum(coef * u) are
 *   zero or at least 2^-969 (2e-292) in magnitude.  The fused passes divide
 *   by the diagonal with a reciprocal and one correction step, whose
 *   remainder must not underflow (tools/check_division.c).  Below 2^-969 a
 *   quotient is within one ulp of the reference's (first seen near 2^-1003,
 *   1e-302); the coarsest solve and smoothers 1 / 2 use the true division, so
 *   down there two kernels of this library may differ from each other by that
 *   ulp on the same point.  A numerator of +-Inf gives NaN where the reference
 *   gives +-Inf; NaN and +-0 give what the reference gives.
 * MGX_FP_FMA: the operator divided by its diagonal and contracted: each
 *   update u = f/d + m_N uN + m_W uW + m_E uE + m_S uS as four fused
 *   multiply-adds (m = -coefficient/d), residuals d*(update - u) -- within a
 *   few ulp per operation of the reference (max|duT| <= 1e-12,
 *   the same cycle counts), independent of the kernel or row partition that
 *   computes a point.  The reference's own GPU build contracts too (nvcc
 *   defaults to -fmad=true, gs.cu). */
#define MGX_FP_BITWISE 0
#define MGX_FP_FMA 1

/* Fills *opt with the reference defaults. */
void mgx_default_options(mgx_options *opt);

/* multigrid.cpp:124-186 with the reference signature: host arrays u0, v1, v2
 * of (n+1)^2 doubles in, uT out.  Runs (int)(T/dt) Crank-Nicolson steps, each
 * compute_rhs + mg_outer, entirely on the GPU. */
int mgx_timestepper(double *uT, const double *u0, const double *v1, const double *v2,
                    double nu, int maxlvl, long n, double dt, double T, double dx,
                    double tol, int shape);
/* Same with options; cycles_per_step (may be NULL) gets mg_outer's cycle count
 * for every step (length (int)(T/dt)). */
int mgx_timestepper_ex(double *uT, const double *u0, const double *v1, const double *v2,
                       double nu, int maxlvl, long n, double dt, double T, double dx,
                       double tol, const mgx_options *opt, int *cycles_per_step);

/* Context: the level towers u/rhs/v1/v2 (multigrid.cpp:131-162) resident in HBM.
 * n = finest N (power of two), maxlvl = number of levels, dt, nu as in
 * timestepper.  Multi-GPU: see mgx_create_dist. */
typedef struct mgx_ctx mgx_ctx;

int mgx_create(mgx_ctx **ctx, long n, int maxlvl, double dt, double nu,
               const mgx_options *opt);
int mgx_destroy(mgx_ctx *ctx);

/* Host <-> device in the reference layout ((n+1)^2 row-major).  upload sets
 * u = u0, v1, v2 on the finest level and builds the coarse velocity tower;
 * download copies the finest u. */
int mgx_upload(mgx_ctx *ctx, const double *u0, const double *v1, const double *v2);
int mgx_download(mgx_ctx *ctx, double *u);
/* Device-pointer variants (reference layout, device memory). */
int mgx_upload_device(mgx_ctx *ctx, const double *u0, const double *v1, const double *v2);
int mgx_download_device(mgx_ctx *ctx, double *u);

/* compute_rhs on the finest level (multigrid.cpp:167). */
int mgx_rhs(mgx_ctx *ctx);
/* `sweeps` RB-GS sweeps on level `level` (gauss_seidel, multigrid.cpp:69-72). */
int mgx_gs(mgx_ctx *ctx, int level, int sweeps);
/* residual + compute_norm on `level` (multigrid.cpp:104-105, 62-63). */
int mgx_residual_norm(mgx_ctx *ctx, int level, double *norm);
/* residual on `level` restricted into rhs[level+1], and u[level+1] = 0
 * (multigrid.cpp:73-77). */
int mgx_restrict(mgx_ctx *ctx, int level);
/* u[level] += prolongation(u[level+1]) (multigrid.cpp:81-83). */
int mgx_prolong_add(mgx_ctx *ctx, int level);
/* One V- (or W-) cycle from the finest level: mg_inner(lvl=0) (multigrid.cpp:17-92). */
int mgx_vcycle(mgx_ctx *ctx);
/* mg_outer (multigrid.cpp:97-120): cycles until ||r||/||r0|| <= tol or the cap.
 * Any output pointer may be NULL.  Returns MGX_E_NOCONV when the cap is hit:
 * whenever *cycles == max_cycle, also when that last allowed cycle reached the
 * tolerance (compare *res / *res0 with tol to tell).  u, *cycles and the norms
 * are then those of the max_cycle cycles, and the context is ready for the next
 * call.  A non-finite initial norm runs no cycle and returns MGX_OK, as the
 * reference's loop does.  mgx_timestepper[_ex] steps on after a capped step. */
int mgx_mg_outer(mgx_ctx *ctx, double tol, int *cycles, double *res0, double *res);
/* One timestep: mgx_rhs + mgx_mg_outer (multigrid.cpp:165-172). */
int mgx_step(mgx_ctx *ctx, double tol, int *cycles);
/* The same step; *res0 / *res (may be NULL) also receive mg_outer's initial and
 * last residual norm, as mgx_mg_outer returns them (the initial one is taken
 * by the pass that forms the right-hand side). */
int mgx_step_ex(mgx_ctx *ctx, double tol, int *cycles, double *res0, double *res);
/* Bench step x `cycles`: V-cycle + residual + norm, no tolerance stop.
 * *res (may be NULL) receives the last residual norm. */
int mgx_run_cycles(mgx_ctx *ctx, int cycles, double *res);

/* Introspection. */
int mgx_level_n(mgx_ctx *ctx, int level, long *n);
/* Copy level `level`'s field (0=u, 1=rhs, 2=v1, 3=v2) to host, reference layout. */
int mgx_download_level(mgx_ctx *ctx, int level, int field, double *out);
/* Number of coarsest-level GS iterations performed since creation. */
int mgx_coarse_iterations(mgx_ctx *ctx, long *iters);
/* The HIP stream (hipStream_t) the context launches on. */
int mgx_stream(mgx_ctx *ctx, void **stream);
/* Waits for all of the context's work; a partitioned context's side-stream
 * exchanges included, so no RCCL operation of it is in flight on return (the
 * caller's own collectives may follow). */
int mgx_synchronize(mgx_ctx *ctx);

/* Process-wide tuning knobs.  "tile_max_n": levels with n <= value run the
 * fused smoothing pass as 2-D LDS tiles instead of the row march (default 1024).
 * "cross_cycle": 1 (default) fuses, inside mg_outer / run_cycles / step, the
 * finest level's post-smoothing of each V-cycle with the pre-smoothing of
 * the next into one HBM pass (levels with n >= 4096, V- and W-cycles -- a
 * W-cycle also fuses its two level-0 visits --, nsmooth 2 or
 * 3; bitwise the same results); after such a cycle the coarse levels hold
 * the next cycle's restricted rhs, not the last correction.  0 = off.
 * "dist_min_rows": partitioned solvers replicate every level whose row blocks
 * would be shorter than this (default 256, even, >= 16); read at creation.
 * "dist_overlap": partitioned contexts, 1 = every partitioned level's u
 * ghost rows are exchanged on a second stream as soon as the pass that wrote
 * them ends, hidden behind the coarser levels (the level's next pass waits for
 * it), and the cross pass's restricted level-1 rhs behind the norm's host
 * round trip; 2 = that, and the cross pass's remaining exchange (level-1 u) on
 * the second stream beside the pass's interior march, the two 16-row bands next
 * to the ghosts after it; 0 = every exchange on the compute stream; -1
 * (default) = 1 on an RCCL communicator, 0 on virtual ranks (one GPU, where
 * the side stream's copies compete with the passes).  Bitwise the same results.
 * Whatever the mode, a rank has ONE communicator and at most one RCCL
 * operation in flight: each is chained after the previous one by an event.
 * "dist_comm_chain": test hook, 1 (default) = that chain; 0 drops it so the
 * fake-RCCL test can show its happens-before check catching the overlap.
 * Never 0 with real peers.
 * "dist_local_side": virtual ranks only: 0 (default) runs the dist_overlap
 * exchanges at their early points on the compute stream (one device: no
 * second link to overlap with), 1 on the second stream as over RCCL.  Bitwise
 * the same results.
 * "xfast": 1 (default) runs the cross-cycle pass as an unguarded kernel over
 * the interior strips and rows plus a guarded kernel over the boundary strips
 * and bands; 0 = one guarded launch (bitwise the same results).
 * "xpack": 1 = the cross-cycle pass hands the next cycle's pre-smoothed u on
 * with one of its two colours only (half-pitch rows, 8 B per point pair) and
 * the next pass rebuilds the other colour -- the pre-smoothing's last
 * half-sweep again, from operands it reads anyway -- so a pass moves one finest
 * array less (half written, half read); 0 = whole rows; 2 (default) = 1
 * inside mgx_run_cycles in fp_mode fma (level 0 -4.8 % at N=16384), else 0:
 * in the bitwise mode the rebuilt colour's division makes the pass 5 %
 * slower, and mg_outer / step end in a pass that needs whole rows, so a
 * packed u_pre would cost them an expansion pass per call.  Bitwise the same
 * results.  Whole levels run as row marches only (not the LDS-tile
 * form of "xtile_max_rows", nor step mode, nor partitioned contexts); a pass
 * that needs whole rows after a packed one (the last cycle's plain
 * post-smoothing, a recomputed u_post) expands it first.
 * "wpack": the levels below the finest whose pre- and post-smoothing both run
 * as wave marches (whole levels, nsmooth 2 or 3 in one pass, not partitioned):
 * 1 = the pre-smoothing stores only the colour its last half-sweep updated
 * (half-pitch rows) and the level's post-smoothing, the buffer's only reader,
 * loads just that: the post-smoothing's first half-sweep overwrites the other
 * colour without reading it, and the Dirichlet ring of these levels is zero,
 * so nothing is rebuilt and each of the two passes moves half a level array
 * less.  0 = whole rows; 2 = 1 in fp_mode fma only.  Bitwise the same results.
 * A post-smoothing that turns out not to be such a march gets whole rows
 * first (the pre-smoothing run again without its restriction); 3 is a test
 * hook: packed as 1, and every post-smoothing takes that expansion.
 * "march_tile_rows": a row block whose wave march would give each resident
 * workgroup fewer than this many rows runs as LDS tiles (default 16, >= 0).
 * "xtile_max_rows": on row blocks of at most this many rows (a rank of a
 * partitioned solver, a small level) the cross-cycle pass runs the boundary
 * strips and bands as LDS tiles instead of the guarded row march (latency
 * bound: ~0.15 ms whatever the block height); default 4097, 0 = never.
 * "march_order": work order of the row marches, bit 0 = band-major (the
 * workgroups of neighbouring strip groups march the same rows at the same
 * time, so their shared halo columns are fetched once; launches with >= 192
 * rows per workgroup), bit 1 = XCD-contiguous workgroup order; default 3.
 * "tile_xcd": 1 (default) deals the LDS tiles
 * XCD-contiguous.  "tile32_min_n": K=3 tile passes on levels n >= value use
 * 32-row tiles (default 2048).  "march_min_rows": fewest rows per workgroup
 * of a wave-march launch (default 32, >= 8).
 * "march_seg": 1 (default) gives each workgroup of a row march one
 * full-height segment when equal shares would leave a short last band whose
 * workgroups march pieces of several strips (row blocks of a partitioned
 * level); 0 = equal shares only.
 * "step_fuse": 1 (default) runs a time step's compute_rhs, mg_outer's initial
 * residual norm and the first cycle's finest pre-smoothing as one pass
 * (single GPU, cross-cycle schedule, row-march finest level); 0 = the rhs and
 * norm pass, then the pre-smoothing (bitwise the same results).
 * "post_predict": mg_outer / step let the cross-cycle pass store a cycle's
 * post-smoothed u (the value returned if that cycle converges) only when the
 * cycle's residual, extrapolated with the last cycle's reduction factor, is
 * within post_predict x tol; a cycle that converges without it is recomputed
 * by one post-smoothing pass (default 10; 0 = always store,
 * -1 = never store: bitwise the same results).
 * "post_only": a cycle of mg_outer / step whose extrapolated norm is within
 * tol / post_only (or the last cycle allowed) runs its finest post-smoothing
 * as a pass of its own instead of the cross-cycle pass (no pre-smoothing of a
 * next cycle that would not run); if it does not converge after all, the next
 * cycle pre-smooths from its result (default 10; 0 = never; -1 = every cycle).
 * "step_cross": 1 (default) lets mgx_step's last cycle (single GPU, whole
 * levels n >= 8192) run the cross-cycle pass in time-step mode: it also
 * forms the next step's rhs, initial norm and first pre-smoothing, which the
 * next mgx_step starts from (any other call in between drops them); 0 = each
 * step starts with its own rhs + norm pass.
 * "coarse_fuse": 1 (default) runs the coarsest solve (n <= 64, with
 * coarse_lds) inside the prolongation tile pass of the level above: every
 * workgroup of that pass solves the coarsest level in its LDS and prolongs
 * from the copy, one stores it -- no coarse launch, bitwise the same results,
 * norms and iteration counts; 0 = its own launch.  Single-GPU contexts and
 * the replicated levels of a partitioned one, when the level above runs as
 * LDS tiles and the coarsest is level 2 or deeper.
 * "coarse_lds": 1 (default) solves coarsest levels n <= 64 with u in LDS
 * and each thread's rhs / v1 / v2 in registers, 0 = through L2 (bitwise the
 * same).  A W-cycle's `shape` consecutive solves of the coarsest level run in
 * one launch either way.
 * "wpair": 1 (default) runs a W-cycle's post-smoothing of one visit and the
 * pre-smoothing of the next visit of an LDS-tile level (nothing runs between
 * them, multigrid.cpp:52) as one tile pass of 2 nsmooth sweeps; 0 = two
 * passes (bitwise the same).
 * None of them changes a bit of u or a cycle count; residual norms taken by
 * a different kernel (cross_cycle, post_only, step_fuse) agree to 1e-11
 * relative (other reduction trees; a cycle count could differ only on a norm
 * that far from tol). */
int mgx_set_tuning(const char *key, long value);
/* "sep_velocity": 1 (default) = a velocity field that is an exact rank-1
 * outer product in floating point, v[i][j] == a[i]*b[j] bitwise (the
 * reference's rotating flow, multigrid.cpp:221-222, is one), is detected at
 * upload and the finest level's cross pass reads its factors instead of the
 * 2-D v1 / v2 (two of its five input streams); 0 = always the 2-D arrays.
 * Bitwise the same results either way.
 * "zero_rows": 1 (default) = at upload, the rows from which every row of a
 * coarse level's v1 and v2 is zero (3/4 of each coarse level of the
 * reference tower) are found, and the row marches read them from
 * one L2-resident zero row instead of HBM; 0 = every row from HBM (bitwise
 * the same results).
 * "vgen": 1 (default) = levels 1-2 of the reference tower, whose v1 / v2 are
 * re-reads of the finest rank-1 field, and every level below the
 * coarsest of the correct tower (strided injections of it: v_l(i, j) =
 * fl(a[2^l i] * b[2^l j])), generate them in the V-cycle's 3-sweep smoothing
 * passes from the finest level's factors instead of reading them from HBM --
 * only when every entry of the level equals the generator's bits (checked at
 * upload, per level; on row blocks per block, ghost rows included); 0 = reads
 * them.  Bitwise the same. */
/* Host only: exact rank-1 factors of v (rows x (n+1), row-major):
 * returns 1 and fills a[rows], b[n+1] with fl(a[i]*b[j]) == v[i][j] (same
 * bits) and every nonzero |v|, |b| still normal after scaling by smin, else 0. */
int mgx_factor_velocity(const double *v, long rows, long n, double smin, double *a, double *b);
/* *factored: a bit mask (since round 4; before, 0 or 1 -- bit 0 keeps that
 * meaning): bit 0 = the context keeps velocity factors for its finest level;
 * bit l (l >= 1) = level l generates its velocity from them ("vgen": levels
 * 1-2 of the reference tower, any level below the coarsest of the correct
 * tower). */
int mgx_velocity_factored(mgx_ctx *ctx, int *factored);
int mgx_get_tuning(const char *key, long *value);
/* Build provenance, fixed when the library was compiled: the sha256 (hex) of
 * the kernel sources (csrc stencil.h, kernels.h, kernels.hip, wsmooth.hip,
 * xsmooth.hip, concatenated in that order -- the key the committed PMC
 * profiles are stamped with) and of every product source (those + ctx.h,
 * plan.h, sepvel.h, mgx.hip, dist.hip, vfactor.h, vfactor.hip, source.h,
 * source.hip, diag.h, diag.hip, boundary.h, boundary.hip, tstep.h, tstep.hip,
 * bdf.h, bdf.hip, errest.h, errest.hip, dense.h, dense.hip, predict.h,
 * predict.hip, include/mgx.h). */
const char *mgx_build_id(void);
const char *mgx_build_sources_id(void);

/* Per-kernel timing with HIP events on the context stream. */
#define MGX_K_GS 0             /* RB-GS sweep (one full red+black sweep) */
#define MGX_K_RESTRICT 1       /* residual restricted to the coarse rhs */
#define MGX_K_PROLONG 2        /* prolongation + add */
#define MGX_K_RESNORM 3        /* residual + norm partials */
#define MGX_K_COARSE 4         /* coarsest-level solve */
#define MGX_K_RHS 5            /* compute_rhs */
#define MGX_K_HALO 6           /* halo exchange (multi-GPU) */
#define MGX_K_PSMOOTH 7        /* prolongation + add fused into a smoothing pass */
#define MGX_K_XSMOOTH 8        /* finest level: post-smoothing of cycle k + pre-smoothing of k+1 */
#define MGX_K_COUNT 9
/* on: 0 off, 1 every launch, 2 finest-level launches only (two events per
 * recorded launch; mode 2 keeps the overhead off the small levels).
 * Partitioned contexts: the replicated levels are recorded in mode 1, and in
 * mode 2 only where everything is replicated (the first replicated level is
 * 0, mgx_dist_info), the finest level then being one of them. */
int mgx_profile_enable(mgx_ctx *ctx, int on);
int mgx_profile_reset(mgx_ctx *ctx);
/* For kernel kind `kind` on level `level` (-1 = all levels): launches, summed
 * device milliseconds, summed algorithmic bytes (SURVEY 8d byte model). */
int mgx_profile_get(mgx_ctx *ctx, int kind, int level, long *launches, double *ms,
                    double *bytes);
/* The same plus the compulsory bytes of those launches: every array a launch
 * reads or writes counted once (the traffic floor of a fused pass, and the
 * roofline denominator bench.py reports). */
int mgx_profile_get_ex(mgx_ctx *ctx, int kind, int level, long *launches, double *ms,
                       double *bytes, double *cbytes);

/* ---- Row-partitioned multi-GPU solver ---------------------------
 * The finest levels are split into contiguous row blocks, one per rank, with
 * ghost rows refreshed once per fused smoothing pass; levels whose blocks
 * would be shorter than 256 rows are replicated on every rank (the restricted
 * rhs is all-gathered).  u after any number of V-cycles is bitwise the
 * single-GPU (and reference) result; the residual norm is an all-reduced sum.
 * A partitioned context takes every whole-solver call (upload/download of the
 * full grid, rhs, vcycle, mg_outer, step, run_cycles, residual_norm at level
 * 0); the per-level calls (gs, restrict, prolong_add, download_level) return
 * MGX_E_ARG.  Needs smoother 0, nsmooth >= 1, world a power of two. */
/* Measured streaming bandwidth (GB/s, read + write bytes) of a 16-B-per-lane
 * grid-stride kernel with `nin` input streams (1: copy; 4: the smoother's
 * shape, 4 in + 1 out) of `bytes_per_stream` each, `reps` launches timed with
 * HIP events: the practical HBM ceiling reported beside the 8 TB/s spec. */
int mgx_stream_bandwidth(long bytes_per_stream, int nin, int reps, double *GBs);

#define MGX_UNIQUE_ID_BYTES 128
/* RCCL unique id (128 bytes) made on one rank and shared with the others. */
int mgx_dist_unique_id(void *id128);
/* One rank of `world` (one process per GPU; select the GPU with opt->device).
 * Collective: every rank must call it with the same id, n, maxlvl, options. */
int mgx_create_dist(mgx_ctx **out, long n, int maxlvl, double dt, double nu,
                    const mgx_options *opt, int rank, int world, const void *id128);
/* `world` virtual ranks in this process on one GPU, ghost exchanges as
 * device copies (tests the partition on a single GPU). */
int mgx_create_local_dist(mgx_ctx **out, long n, int maxlvl, double dt, double nu,
                          const mgx_options *opt, int world);
/* Partition plan (host only): owned rows [*ra, *rb) of `level` on `rank`, and
 * the first replicated level (levels >= it are whole on every rank). */
int mgx_partition(long n, int maxlvl, int world, int rank, int level, int *ra, int *rb,
                  int *replicated_level);
/* Host-only: the ghost-row exchange plan of `rank` on `level` (both transports
 * execute it).  *count entries of 5 ints: peer, send_row, send_rows, recv_row,
 * recv_rows (global rows of the level: send rows [send_row, +send_rows) to
 * peer, receive rows [recv_row, +recv_rows) from it); 0 entries on replicated
 * levels or world 1.  cap = room in xfers (entries). */
int mgx_exchange_plan(long n, int maxlvl, int world, int rank, int level, int *count,
                      int *xfers, int cap);
/* Host-only: the all-gather into the first replicated level *level: `rank`
 * contributes rows [*row0, *row0 + *rows) of its restricted rhs (in place,
 * rank-major, equal counts). */
int mgx_gather_plan(long n, int maxlvl, int world, int rank, int *level, int *row0,
                    int *rows);
/* Allocated rows [*lo, *hi] (owned + ghosts) of the finest level of local part
 * `part` (0 on an RCCL rank; 0..world-1 for mgx_create_local_dist). */
int mgx_dist_rows(mgx_ctx *ctx, int part, int *lo, int *hi);
/* Row-block upload, so that no rank ever holds the whole grid (SURVEY 8e C5:
 * N=65536 on 8 GPUs): u0[i], v1[i], v2[i] hold rows [lo, hi] (mgx_dist_rows)
 * of local part i, (hi-lo+1)*(N+1) doubles each.  The velocity tower is built
 * on the device from the row blocks, which needs MGX_TOWER_CORRECT (the
 * reference tower reads the whole grid).  Collective. */
int mgx_upload_rows(mgx_ctx *ctx, const double *const *u0, const double *const *v1,
                    const double *const *v2);
/* Owned finest-level rows [*ra, *rb) of local part `part` (the last rank also
 * owns the boundary row N; a single-GPU context: part 0 = [0, N+1)). */
int mgx_owned_rows(mgx_ctx *ctx, int part, int *ra, int *rb);
/* Row-block download, the counterpart of mgx_upload_rows: the owned rows of
 * local part `part` into rows[(rb-ra)*(N+1)], reference layout.  No
 * communication and no whole-grid buffer on any rank (C5: N=65536). */
int mgx_download_rows(mgx_ctx *ctx, int part, double *rows);
/* The reference's uT text output (multigrid.cpp:269-284, "%d\t%d\t%f\n", i
 * outer, j inner) for rows [r0, r1) held in rows[(r1-r0)*(N+1)]; append != 0
 * appends.  Rank-ordered appends of each rank's owned rows give the file the
 * whole-grid writer gives, byte for byte.  nthreads <= 0: all host threads. */
int mgx_write_uT(const char *path, const double *rows, long N, long r0, long r1, int append,
                 int nthreads);
/* world size, rank (-1 for a local multi-part context; 0/1 for single GPU),
 * first replicated level (maxlvl for a single-GPU context). */
int mgx_dist_info(mgx_ctx *ctx, int *world, int *rank, int *replicated_level);

/* ---- Device-resident and time-dependent velocity fields ---------------------
 * Tuning key "device_factor": which uploads find the exact rank-1 factors of
 * v1 / v2 ("sep_velocity") with the device verifier (csrc/vfactor.hip, part of
 * mgx_build_sources_id) on the context's own copy of the fields: 1 (default)
 * = uploads from device pointers (mgx_upload_device, mgx_set_velocity_device,
 * partitioned contexts built from them), 2 = uploads from host pointers too
 * (after their copy), 0 = none: a device upload keeps the 2-D arrays and runs
 * the generic passes.  The host and the device backend return the same
 * factors; u, norms and cycle counts do not depend on the key.
 * (Read-only, mgx_get_tuning: "vfactor_rounds" / "vfactor_us" = the check-
 * kernel launches of the calling thread's last device factorisation of one
 * field and their summed device microseconds, for measurements.) */
/* Device counterpart of mgx_factor_velocity: v (rows x (n+1), row stride ld
 * doubles), a[rows], b[n+1] are DEVICE pointers; *factored = 1 and a, b filled
 * with the same bits the host function returns for the same field, else 0.
 * Null stream; synchronises. */
int mgx_factor_velocity_device(const double *v, long rows, long n, long ld,
                               double smin, double *a, double *b, int *factored);
/* Replace the velocity of a single-GPU context and keep the finest-level u:
 * equivalent, bit for bit in everything that follows, to downloading u and
 * calling mgx_upload(ctx, u, v1, v2).  Host / device pointers, reference layout.
 * The coarse velocity tower, its zero rows, the factors and the generating
 * levels are rebuilt; the rhs, a pending next step and captured sub-cycles of
 * the old velocity are dropped (call mgx_rhs or mgx_step next).  A partitioned
 * context returns MGX_E_ARG. */
int mgx_set_velocity(mgx_ctx *ctx, const double *v1, const double *v2);
int mgx_set_velocity_device(mgx_ctx *ctx, const double *v1, const double *v2);

/* ---- Source term: u_t + v.grad u = nu lap u + f -----------------------------
 * With a source f and a scale s (default 1) set on a context, every
 * finest-level compute_rhs of that context -- mgx_rhs and the start of
 * mgx_step -- gives at every interior point
 *     rhs(i,j) = fl( Bu(i,j) + fl( c * f(i,j) ) ),   c = fl(dt * s),
 * Bu being exactly what compute_rhs gives without a source (gs.cpp:24-53); no
 * contraction in either fp_mode, boundary entries untouched.  f has the
 * reference layout ((n+1)^2 row-major); its boundary entries are ignored.  For
 * second-order Crank-Nicolson pass f at the half step: which f is the
 * caller's business.  Everything else on such a context, everything on a
 * context without a source, mgx_timestepper[_ex] and mgx_compute_rhs are
 * unchanged.
 *
 * mgx_set_source takes a host pointer, mgx_set_source_device a device pointer.
 * The context keeps its own pitched copy (one more finest-level array): the
 * caller's buffer is free on return, with the ordering rules of
 * mgx_upload[_device].  f == NULL removes the source and frees the copy: from
 * the next call on the context behaves, bit for bit and pass for pass, as if
 * none had ever been set.  When the copy cannot be allocated (N=65536 on one
 * GPU has no room for another finest-level array) the call returns MGX_E_HIP
 * with a message and leaves the context without a source.
 * mgx_set_source_scale sets s: a time-separable source g(t) f(x,y) costs
 * nothing per step beyond the call.  The source and the scale survive
 * mgx_upload* and mgx_set_velocity*; only NULL or mgx_destroy removes the
 * source.  Setting, replacing, rescaling or removing it drops whatever was
 * formed from the old right-hand side (a pending next step, a speculative
 * pre-smoothed u), as mgx_set_velocity does: call mgx_rhs or mgx_step next.
 *
 * The pass (csrc/source.hip, part of mgx_build_sources_id; profile kind
 * MGX_K_RHS) is one row march that reads u, v1, v2 and f and writes rhs, for
 * mgx_step also mg_outer's initial norm -- bitwise what mgx_rhs followed by
 * mgx_residual_norm(ctx, 0) gives.  Tuning key "source_sv": 1 (default) = on a
 * context that keeps finest-level velocity factors (bit 0 of
 * mgx_velocity_factored) the pass forms v1, v2 from them instead of reading
 * the 2-D arrays (three full streams instead of five; bitwise the same); 0 =
 * always the 2-D arrays.
 * Cost: while a source is set, mgx_step does not fuse the right-hand side into
 * the first pre-smoothing pass ("step_fuse") or into the previous step's last
 * cross-cycle pass ("step_cross"), which form it inside kernels that know no
 * source; every step starts with the pass above.  The cycles themselves
 * (cross_cycle included) are unchanged.  Measured on one MI355X (DESIGN.md
 * section 9): a source costs about 2.9 ms per step at N=16384, L=9, fma (11.1
 * against 8.2 ms, three cycles per step; 3.7 ms with "source_sv" 0).
 *
 * Partitioned contexts (mgx_create_local_dist, mgx_create_dist) take the
 * whole-grid calls: each part keeps its owned rows, and no exchange is added
 * (the term is pointwise).
 *
 * Separable and row-block sources.  A context has ONE source: a field (set by
 * mgx_set_source or, row block by row block, by mgx_set_source_rows) or a
 * separable one (mgx_set_source_separable).  Setting either kind replaces the
 * other and frees a field copy; mgx_set_source(ctx, NULL) removes whichever is
 * set.  The scale, the survival across mgx_upload* and mgx_set_velocity*, the
 * dropped state and mgx_source_info (active = 1 for either kind) are those
 * described above; mgx_source_kind tells the kinds apart.
 *
 * mgx_set_source_separable[_device]: the source is a short sum of outer
 * products, 1 <= terms <= MGX_SOURCE_MAX_TERMS, given by its factors a[r][0..N]
 * (rows) and b[r][0..N] (columns), term-major:
 *     f(i,j) = t_0                                  for one term,
 *     f(i,j) = fl( ... fl( fl(t_0 + t_1) + t_2 ) ... )   left to right,
 *     t_r    = fl( a[r][i] * b[r][j] ),
 * then rhs = fl(Bu + fl(c * f)) as above, never contracted: bit for bit what
 * mgx_set_source gives for the array built in that order (numpy: f =
 * a[0][:,None]*b[0][None,:], then f = f + a[r][:,None]*b[r][None,:]).
 * Boundary entries of a and b are ignored.  The pass forms f in registers: no
 * finest-level array is allocated (the call cannot fail for room at N=65536),
 * no f stream is read, and mg_outer's initial norm is bitwise that of the
 * field pass on the same f.  The context keeps its own copies of the factors
 * (8(N+1) bytes per vector); replacing the factors of a separable source that
 * is set reuses them -- the per-step call of a moving emitter, about 1 MB at
 * N=16384 with four terms.  It works on every kind of context: a single GPU,
 * local parts and RCCL ranks, filled by mgx_upload or mgx_upload_rows; every
 * part keeps the factors and no exchange is added.  On RCCL ranks every rank
 * must pass the same values: the call does not communicate, so a mismatch
 * cannot hang -- it gives a right-hand side no single source describes.
 * Field 4 of mgx_field_stats* / mgx_sample* returns MGX_E_ARG on a separable
 * source (no copy of f is kept).
 *
 * mgx_set_source_rows[_device]: the row-block counterpart of mgx_set_source for
 * contexts on which no rank holds the whole grid (mgx_upload_rows): f[i] holds
 * the OWNED rows [ra, rb) (mgx_owned_rows) of local part i, (rb-ra)*(N+1)
 * doubles, reference layout.  All parts or none on an allocation failure.  A
 * partitioned context with no partitioned level returns MGX_E_ARG (use
 * mgx_set_source, as mgx_upload_rows asks for mgx_upload); on a single-GPU
 * context part 0 is all rows and the call is mgx_set_source(ctx, f[0]).
 *
 * Profile accounting (kind MGX_K_RHS): the separable pass's compulsory bytes
 * are 16 per point with velocity factors ("source_sv" 1: u in, rhs out), 32
 * without (u, v1, v2, rhs), against 24 / 40 of the field pass; its algorithmic
 * bytes are those of the source-free pass.  Measured on one MI355X (DESIGN.md
 * section 9, N=16384): 0.95 ms against 1.29 ms for the field pass with
 * velocity factors, the same for 1, 2 and 4 terms; mgx_step still does not
 * fuse the right-hand side while any source is set (see above). */
#define MGX_SOURCE_MAX_TERMS 4
int mgx_set_source(mgx_ctx *ctx, const double *f);
int mgx_set_source_device(mgx_ctx *ctx, const double *f);
int mgx_set_source_scale(mgx_ctx *ctx, double s);
/* *active = 1 while a source is set, *scale = s (either may be NULL). */
int mgx_source_info(mgx_ctx *ctx, int *active, double *scale);
/* The gs.h-style raw op: rhs = fl(compute_rhs(u) + fl(c * f)) on the interior,
 * device pointers in the reference layout, null stream (as mgx_compute_rhs);
 * c is the factor itself (a context passes fl(dt * s)). */
int mgx_compute_rhs_source(double *rhs, const double *u, long n, const double *v1,
                           const double *v2, double k, double nu, double h, const double *f,
                           double c);
/* a, b: terms x (N+1) doubles each, term-major.  Host / device pointers. */
int mgx_set_source_separable(mgx_ctx *ctx, int terms, const double *a, const double *b);
int mgx_set_source_separable_device(mgx_ctx *ctx, int terms, const double *a, const double *b);
/* f[i]: the OWNED rows [ra, rb) (mgx_owned_rows) of local part i,
 * (rb-ra)*(N+1) doubles, reference layout.  Host / device pointers. */
int mgx_set_source_rows(mgx_ctx *ctx, const double *const *f);
int mgx_set_source_rows_device(mgx_ctx *ctx, const double *const *f);
/* *kind: 0 none, 1 field (whole-grid or row blocks), 2 separable; *terms: R or 0
 * (either may be NULL). */
int mgx_source_kind(mgx_ctx *ctx, int *kind, int *terms);
/* The raw op with a separable source (device pointers, null stream): a, b hold
 * terms x (n+1) doubles, term-major. */
int mgx_compute_rhs_source_separable(double *rhs, const double *u, long n, const double *v1,
                                     const double *v2, double k, double nu, double h,
                                     int terms, const double *a, const double *b, double c);

/* ---- Field diagnostics: statistics and strided samples on the device --------
 * A context keeps its fields in HBM; these calls look at one without moving
 * it (csrc/diag.hip, part of mgx_build_sources_id): one reduction pass over
 * the field gives the record below, a gather kernel a coarse picture.  No
 * floating-point atomics: the order of every addition is a fixed function of
 * the grid size and the row range, so two calls give the same bits.  Every
 * call here checks its arguments before any device call and reports
 * MGX_E_ARG with a message that starts with its own name.  None of them
 * changes a pass of a context that never calls them, and like the downloads
 * they leave a pending next step or a speculative pre-smoothed u alone.
 * Measured on one MI355X: mgx_field_stats of u at
 * N=16384 takes 0.38 ms of device time (0.74 ms with minus), mgx_sample at
 * stride 64 0.05 ms, against 136 ms for mgx_download alone. */
typedef struct mgx_stats {
    long   count;        /* points examined */
    long   nonfinite;    /* NaN or +-Inf among them */
    double sum, sum_abs, sum_sq;   /* over the FINITE values: x, |x|, fl(x*x) */
    double min, max;     /* over the finite values; +Inf / -Inf when there is none */
    long   min_i, min_j, max_i, max_j;  /* global (row, column) of the first occurrence
                                           in row-major order; -1 when there is none */
} mgx_stats;
/* min and max compare by value (-0 == +0); among equal values the first in
 * row-major order wins and min / max carry that element's bits -- what
 * np.argmin / np.argmax give on the finite entries.
 *
 * The gs.h-style raw op: device pointers in the reference layout ((n+1)^2
 * row-major), any n >= 1, null stream; synchronises (like mgx_compute_norm).
 * minus != NULL: the statistics of d = fl(a - minus), point by point.
 * interior_only = 1: rows and columns 1..n-1 only (count (n-1)^2). */
int mgx_array_stats(const double *a, const double *minus, long n, int interior_only,
                    mgx_stats *out);
/* The statistics of what mgx_download_level(level, field) would return, on the
 * context's stream.  field 0..3 as there, 4 = the context's copy of the source
 * (level 0; MGX_E_ARG when none is set), 5 = the history h and 6 = the second
 * history array h2 (level 0; MGX_E_ARG when that array is absent or not valid
 * -- mgx_set_history, mgx_set_history_depth; the only way to look at the
 * history without a step).  minus: a device pointer in the
 * reference layout of that level, or NULL.  A local-parts context
 * (mgx_create_local_dist) takes level 0 only: the result is mgx_stats_merge of
 * its parts' owned-row results in part order (of sub-context 0 when every
 * level is replicated).  An RCCL rank returns MGX_E_ARG: it performs no
 * communication -- call mgx_field_stats_rows and merge the ranks' records. */
int mgx_field_stats(mgx_ctx *ctx, int level, int field, int interior_only, const double *minus,
                    mgx_stats *out);
/* The owned finest-level rows [ra, rb) (mgx_owned_rows) of local part `part`,
 * with global positions; minus_rows holds those rows only, (rb-ra)*(N+1)
 * doubles on the device, or NULL.  No communication; any context (a
 * single-GPU context has part 0 = all rows).  What an RCCL rank calls. */
int mgx_field_stats_rows(mgx_ctx *ctx, int part, int field, int interior_only,
                         const double *minus_rows, mgx_stats *out);
/* Host only (no HIP call): *into = the record of the union.  Counts and sums
 * add; min / max by value, ties to the smaller (i, j) in row-major order; an
 * operand without a finite value leaves the other's extrema unchanged. */
int mgx_stats_merge(mgx_stats *into, const mgx_stats *other);
/* out[a*(m+1)+b] = field(a*stride, b*stride), m = n/stride: bitwise the
 * entries [::stride, ::stride] of mgx_download_level.  stride must divide the
 * level's n (1 <= stride <= n).  mgx_sample: host `out` (a gather kernel into
 * a compact device buffer, then one copy); mgx_sample_device: device `out`,
 * written by the kernel.  Local-parts contexts: level 0, each part its owned
 * rows; an RCCL rank returns MGX_E_ARG (use mgx_sample_rows). */
int mgx_sample(mgx_ctx *ctx, int level, int field, long stride, double *out);
int mgx_sample_device(mgx_ctx *ctx, int level, int field, long stride, double *out);
/* The sampled rows i in [ra, rb) with i % stride == 0 of local part `part`
 * into the host array out[*rows * (N/stride+1)]; *first_row = the global
 * fine-grid index of the first of them.  out == NULL only reports first_row
 * and rows.  Any context, no communication. */
int mgx_sample_rows(mgx_ctx *ctx, int part, int field, long stride, double *out,
                    long *first_row, long *rows);
/* (Read-only, mgx_get_tuning, beside "vfactor_us": "stats_us" / "stats_bytes"
 * = the device microseconds -- HIP events around the reduction launches only
 * -- and the compulsory bytes of the calling thread's last statistics call.) */

/* ---- Time-dependent Dirichlet data: the ring of u on a live context ---------
 * The boundary values of the finest u are data: every pass reads them and
 * carries them from its input to its output, none computes them.  These calls
 * replace them without moving u off the device (csrc/boundary.hip, part of
 * mgx_build_sources_id).
 *
 * g holds 4(N+1) doubles, side-major:
 *     g[0*(N+1)+j] = u(0,j)    g[2*(N+1)+i] = u(i,0)
 *     g[1*(N+1)+j] = u(N,j)    g[3*(N+1)+i] = u(i,N)
 * The four corners belong to the two row sides: entries 0 and N of sides 2
 * and 3 are ignored on input, and mgx_get_boundary fills them with the corner
 * values.
 *
 * when = MGX_BC_NOW: the ring of the finest u is overwritten now; every other
 * bit of u and the whole right-hand side stay as they are.  What was formed
 * with the old ring is dropped, as by mgx_set_source: a speculative
 * pre-smoothed u, a pending next step, the cross pass's bookkeeping, and a
 * deferred coarsest solve; a packed pre-smoothed u is expanded first.
 * Captured sub-cycles stay (they hold no finest-level value).  g == NULL is
 * MGX_E_ARG.
 *
 * when = MGX_BC_NEXT_STEP: the context copies g (its own device copy,
 * allocated by the first call) and marks it pending.  The next mgx_step or
 * mgx_step_ex consumes it: that step is, bit for bit and cycle count for cycle
 * count,
 *     mgx_rhs(ctx);  mgx_set_boundary(ctx, g, MGX_BC_NOW);  mgx_mg_outer(ctx, ...)
 * -- Crank-Nicolson's rhs = B u^n with the old ring g^n, then A u^(n+1) = rhs
 * with the new ring g^(n+1), mg_outer taking its initial norm after the ring
 * is written.  That step runs the plain schedule (no rhs + norm + pre-smoothing
 * fusion) and prepares no next step; steps with nothing pending run exactly
 * what they ran before.  Setting a ring drops a prepared next step at once.
 * g == NULL cancels a pending ring.  A pending ring survives
 * mgx_set_velocity* and mgx_set_source*; mgx_upload*, mgx_upload_rows and
 * mgx_destroy cancel it.
 *
 * Every kind of context takes mgx_set_boundary*: local parts and RCCL ranks
 * write the two column entries of every row they hold (ghost rows included)
 * and rows 0 / N where they hold them; with every level replicated each
 * sub-context is written.  No communication: every RCCL rank passes the same
 * values, as with mgx_set_source_separable.  mgx_get_boundary* serves
 * single-GPU and local-parts contexts; an RCCL rank returns MGX_E_ARG (it
 * would need communication: use mgx_download_rows or mgx_sample_rows).
 * mgx_boundary_info: *pending = 1 while a MGX_BC_NEXT_STEP ring waits.
 *
 * Every call here checks its arguments before any device call and reports
 * MGX_E_ARG with a message that starts with its own name.  A context that
 * never calls them, and mgx_timestepper[_ex], launch what they launched
 * before.
 * Measured on one MI355X (DESIGN.md section 11, N=16384, L=9, fma, three
 * cycles per step): a step with a device ring set every step takes 12.9 ms
 * against 8.0 ms for the plain step -- 4.9 ms for the plain schedule (its own
 * rhs pass and initial norm, no step fusion, no prepared next step); the ring
 * write itself is 7 microseconds.  mgx_download_device, a ring edit and
 * mgx_upload_device before every step, the only route before, take 28.5 ms
 * per step.  The read-only tuning key "boundary_us" (mgx_get_tuning) gives the
 * device microseconds of the calling thread's last ring write (HIP events
 * around its launches). */
#define MGX_BC_NOW 0
#define MGX_BC_NEXT_STEP 1
int mgx_set_boundary(mgx_ctx *ctx, const double *g, int when);          /* host g   */
int mgx_set_boundary_device(mgx_ctx *ctx, const double *g, int when);   /* device g */
int mgx_get_boundary(mgx_ctx *ctx, double *g);                          /* host out   */
int mgx_get_boundary_device(mgx_ctx *ctx, double *g);                   /* device out */
int mgx_boundary_info(mgx_ctx *ctx, int *pending);
/* The gs.h-style raw op: device pointers, u in the reference layout ((n+1)^2
 * row-major), any n >= 1, null stream: the ring of u = g (layout above), the
 * interior untouched. */
int mgx_write_boundary(double *u, long n, const double *g);

/* ---- Per-step dt and theta on a live context ---------------------------------
 * mgx_create fixes dt, and every step is Crank-Nicolson.  mgx_set_time_step
 * changes both for every later call, without touching the towers: a step
 * becomes the theta-scheme
 *     (I + theta dt L) u^(n+1) = (I - (1 - theta) dt L) u^n + dt f,
 * theta = 1/2 Crank-Nicolson, theta = 1 implicit Euler (a few of which, at
 * dt/2, damp the ringing Crank-Nicolson shows on non-smooth data: Rannacher
 * start-up).  dt is finite and > 0, theta finite with 0 < theta <= 1; anything
 * else is MGX_E_ARG, reported before any device call with a message that
 * starts with the function's name.  A context that never calls it has theta =
 * 0.5 and the dt of mgx_create.
 *
 * Meaning, bit for bit.  With the C doubles
 *     kA = (2.0 * theta) * dt      kB = (2.0 * (1.0 - theta)) * dt
 * (each product rounded, no contraction), from the call on
 *   - every finest-level compute_rhs of the context (mgx_rhs, the start of
 *     mgx_step) is the reference's compute_rhs with k = kB;
 *   - everything that applies or inverts A on any level -- mgx_gs,
 *     mgx_residual_norm, mgx_restrict, mgx_vcycle, mgx_mg_outer,
 *     mgx_run_cycles, the coarsest solve -- is the reference's with k = kA.
 * At theta = 0.5, kA == kB == dt exactly: mgx_set_time_step(ctx, dt of
 * mgx_create, 0.5) changes no bit of anything that follows.  The source weight
 * stays c = fl(dt * s) with the new dt (not kA or kB).  fp_mode fma contracts
 * the kA operator exactly as it contracts today's; the right-hand side and
 * mg_outer's initial norm stay in the reference's term order.  The residual
 * norms mgx_step_ex returns are within 1e-11 relative of the exact norm of the
 * stored fields, as everywhere.
 *
 * The call drops what was formed with the old coefficients -- what
 * mgx_set_boundary(MGX_BC_NOW) drops (a speculative pre-smoothed u, a packed
 * one expanded first; a prepared next step; the cross pass's bookkeeping; a
 * deferred coarsest solve) and the captured sub-cycles of "graph_level", whose
 * nodes hold the coefficients as kernel arguments.  It keeps u, the right-hand
 * side, the velocity tower and its factors, a source and its scale, and a
 * pending ring; the setting belongs to the context and survives mgx_upload*
 * and mgx_set_velocity*.
 *
 * Schedule.  While kA == kB (as doubles) every schedule runs what it ran
 * before, launch for launch (a step right after the call only lacks the
 * prepared next step it dropped).  Otherwise mgx_step starts with one pass of
 * its own (csrc/tstep.hip, part of mgx_build_sources_id; profile kind
 * MGX_K_RHS): rhs = B(kB) u, plus the source term of a field or separable
 * source, and in the same march the norm of rhs - A(kA) u -- bitwise mgx_rhs
 * followed by mgx_residual_norm(ctx, 0).  Its algorithmic bytes are those of
 * the fused rhs + norm pass, its compulsory bytes 16 / 32 per point with /
 * without velocity factors, plus 8 with a field source.  "step_fuse" and
 * "step_cross" are off for such a context: their kernels form the right-hand
 * side and smooth with one set of coefficients (the same reason as for a
 * source).  The cross-cycle pass inside mg_outer stays on.
 *
 * Every kind of context takes the call: local parts and RCCL ranks set every
 * part and every replicated sub-context.  No communication: RCCL ranks pass the
 * same values, as with mgx_set_source_separable.  mgx_timestepper[_ex] and the
 * raw gs.h ops are untouched.
 * mgx_time_step_info: the current dt and theta (either pointer may be NULL). */
int mgx_set_time_step(mgx_ctx *ctx, double dt, double theta);
int mgx_time_step_info(mgx_ctx *ctx, double *dt, double *theta);

/* ---- Variable-step BDF2 steps on a device-resident history --------------------
 * theta = 1/2 is second order but rings on non-smooth data; theta = 1 damps but
 * is first order.  BDF2 is second order and L-stable, and with dt changing per
 * step (mgx_set_time_step) it is the variable-step form, which needs u^(n-1).
 * mgx_set_history(ctx, 1) gives the context one more finest-level array h (one
 * per part of a partitioned context) that holds u^n while u becomes u^(n+1).
 * The same array is the way back from a rejected step (mgx_rollback) without a
 * download before every step.
 *
 * Meaning, bit for bit.  All C doubles, every operation rounded, nothing
 * contracted in either fp_mode (mgx_bdf2_coefficients returns them; host only,
 * any output pointer may be NULL; a non-finite or non-positive dt or dt_prev
 * is MGX_E_ARG):
 *     w  = dt / dt_prev        p = 1.0 + w        q = 1.0 + 2.0 * w
 *     g  = p / q               b0 = (p * p) / q   b1 = (w * w) / q
 *     kA = (2.0 * g) * dt      c  = (g * dt) * s        (s: mgx_set_source_scale)
 * A BDF2 step is, on the interior (boundary entries of rhs untouched),
 *     rhs(i,j) = fl( fl(b0*u(i,j)) - fl(b1*h(i,j)) )
 *                [ then fl(that + fl(c*f(i,j))) with a source, f formed exactly
 *                  as stated for mgx_set_source* above ]
 * followed by mg_outer with the reference's solve operator at k = kA, that is
 * A = I + g dt L.  Constant steps give g = 2/3, b0 = 4/3, b1 = 1/3.  dt is the
 * context's (mgx_set_time_step), dt_prev the dt of the step that made the
 * history.  Zero-stability needs w < 1 + sqrt(2); that is the caller's
 * business and nothing is refused.
 *
 * mgx_set_history(ctx, on): on = 1 allocates h, all parts or none -- on failure
 * MGX_E_HIP with a message, and the context stays without a history (N=65536
 * on one GPU has no room); on a context that has one it is a no-op and keeps
 * its validity.  on = 0 frees it.  A context that never calls it launches
 * exactly what it launches without this section.
 * mgx_history_info: whether a history is on, whether it is valid (holds u^n of
 * a step), the dt of that step, and k_solve, the k every solve-side call of
 * the context currently uses.  Any pointer may be NULL.
 *
 * While a history is on, every mgx_step, mgx_step_ex and mgx_step_bdf2 begins
 * by making h equal to what mgx_download would return at that moment (u^n with
 * ring and corners, before a pending ring is written), and sets dt_prev = dt,
 * valid = 1.  mgx_step[_ex] gives, bit for bit and cycle for cycle, what it
 * gives without a history (one device copy goes ahead of the step), but
 * prepares no next step: "step_cross" is off while a history is on, for the
 * reason a source turns it off -- the next step may be a BDF2 one.
 *
 * mgx_step_bdf2(ctx, tol, cycles, res0, res) (outputs may be NULL; returns
 * MGX_E_NOCONV as mgx_step does): MGX_E_ARG before any device call, with a
 * message that starts with the function's name, for a NULL ctx, a context
 * without a history, and a history that is not valid (a theta-step starts
 * it).  Where kA differs from k_solve it drops what mgx_set_time_step drops
 * (a packed pre-smoothed u expanded first, with the operator that packed it)
 * and rebuilds every level's coefficients.  Then ONE pass (csrc/bdf.hip, part
 * of mgx_build_sources_id; profile kind MGX_K_RHS) stores rhs, stores u over h
 * on the whole array and takes the norm of rhs - A(kA) u, bitwise what
 * mgx_residual_norm(ctx, 0) returns right after; one launch plus the norm's
 * final reduction, on a single GPU and per part.  A ring pending from
 * MGX_BC_NEXT_STEP is written after the pass, and mg_outer then takes its own
 * initial norm, as mgx_step orders it.  mg_outer runs with kA; no next step is
 * prepared.  k_solve stays kA until the next mgx_rhs, mgx_step[_ex] or
 * mgx_set_time_step, each of which re-establishes the theta-scheme's
 * coefficients before anything else.
 * Profile accounting of the pass: compulsory bytes 32 per finest point with
 * velocity factors (u in, h in, h out, rhs out), 48 without, plus 8 with a
 * field source; algorithmic bytes 88, plus 8 with a field source.  Measured at
 * N=16384 (one MI355X, fma, velocity factors): the pass 1.51 ms against 4.16 ms
 * for rhs + device copy + norm; a BDF2 step 11.4 ms, a theta = 1/2 step on the
 * same context 10.9 ms, without a history 8.2 ms.
 *
 * Validity is cleared by mgx_upload*, mgx_upload_rows, mgx_rollback and
 * mgx_set_history(ctx, 0); it is kept by mgx_set_velocity*, mgx_set_source*,
 * mgx_set_boundary* and mgx_set_time_step -- keeping it across a dt change is
 * the point.
 *
 * mgx_rollback(ctx): MGX_E_ARG without a valid history.  Otherwise u becomes h,
 * ring included (a device copy), what mgx_set_boundary(MGX_BC_NOW) drops is
 * dropped and valid is cleared: u^(n-1) is gone, so the next step is a
 * theta-step.  From then on the context behaves, bit for bit, as a twin that
 * was given u^n by mgx_upload with the same velocity, source and settings.
 * The right-hand side is stale afterwards: call mgx_step next.
 *
 * Every kind of context takes all of this: local parts and RCCL ranks keep one
 * h per part (the owned rows are the history; the pass is pointwise plus the
 * norm the partitioned step already takes, so no exchange is added), and with
 * every level replicated each sub-context keeps its own.  mgx_timestepper[_ex]
 * is untouched.
 *
 * Raw op mgx_compute_rhs_bdf2: device pointers, reference layout, any n >= 2,
 * null stream; f may be NULL.  The expression above on the interior of rhs;
 * nothing else is written. */
int mgx_bdf2_coefficients(double dt, double dt_prev, double *g, double *b0, double *b1,
                          double *kA);
int mgx_set_history(mgx_ctx *ctx, int on);
int mgx_history_info(mgx_ctx *ctx, int *on, int *valid, double *dt_prev, double *k_solve);
int mgx_step_bdf2(mgx_ctx *ctx, double tol, int *cycles, double *res0, double *res);
int mgx_rollback(mgx_ctx *ctx);
int mgx_compute_rhs_bdf2(double *rhs, const double *u, const double *h, long n, double b0,
                         double b1, const double *f, double c);

/* ---- Step error estimate on a two-deep history --------------------------------
 * An adaptive loop needs a measure of a step's error and a way back that does
 * not lose second order.  mgx_set_history_depth(ctx, 2) gives the context a
 * second history array h2 in the layout of h (one per part / sub-context, as
 * h), so that after a step u = u^(n+1), h = u^n and h2 = u^(n-1) are resident
 * together; mgx_step_error turns them into the record below in one reduction
 * pass (csrc/errest.hip, part of mgx_build_sources_id).
 *
 * mgx_set_history_depth(ctx, depth): 0 = mgx_set_history(ctx, 0), 1 = the
 * history of the section above, 2 = h and h2; anything else MGX_E_ARG.
 * Allocation is all parts or none: on failure MGX_E_HIP with a message, and
 * the context keeps the depth it had.  1 -> 2 keeps h and its validity, with
 * valid2 = 0; 2 -> 1 frees h2.  mgx_set_history(ctx, 1) on a context that has a
 * history leaves its depth alone, mgx_set_history(ctx, 0) frees everything.
 * mgx_history_depth: the depth, whether h2 is valid, and dt_prev2, the dt of
 * the step that started from h2.  Any pointer may be NULL.
 *
 * At depth 2 every mgx_step, mgx_step_ex and mgx_step_bdf2 ends with h = u^n
 * as at depth 1 and h2 = what h held, valid2 = what valid was, dt_prev2 = what
 * dt_prev was.  No data is copied for this: the step's snapshot is written into
 * the older buffer and the two pointers are exchanged -- a theta-step's device
 * copy goes into the old h2 buffer, and the BDF2 pass reads u^(n-1) from h and
 * stores u^n into the other buffer, the bytes it moves at depth 1, where both
 * pointers are the same address and the pass gives the same bits.  valid2 is
 * cleared wherever valid is.  A context that never calls
 * mgx_set_history_depth launches and returns exactly what it does without
 * this section.
 *
 * mgx_rollback at depth 2: u = h as at depth 1, with the same drops.  Then, if
 * valid2, the pointers are exchanged: h = u^(n-1), dt_prev = dt_prev2, valid
 * stays 1, valid2 = 0 -- the retry may be mgx_step_bdf2 at any dt, second
 * order.  Without valid2 it is the rollback of depth 1.  A second mgx_rollback
 * before the next step is MGX_E_ARG: h is then not the u to go back to.
 *
 * The record.  All C doubles, every operation rounded, nothing contracted in
 * either fp_mode, the division the true one.  On the host w = dt_prev /
 * dt_prev2 and p = 1.0 + w.  At every interior point (rows and columns
 * 1..n-1):
 *     up = fl( fl(p*h) - fl(w*h2) )       linear extrapolation of u^(n-1), u^n
 *                                         to t^(n+1)
 *     d  = fl( u - up )
 *     c  = fl( u - h )
 *     sc = fl( atol + fl( rtol * max(|u|, |h|) ) )
 *     e  = d / sc
 * Conventions of mgx_stats: the sums are of fl(x*x), the maxima of |x|; for
 * err_max the record gives the global position of the first occurrence in
 * row-major order; the position is -1 and the three maxima are -Inf when no
 * point is finite.  A point whose e is NaN or +-Inf counts in `nonfinite` and
 * in nothing else (atol = 0 where u = h = 0 is such a point).  No
 * floating-point atomics: the order of every addition is a fixed function of
 * N and the row range, so two calls give the same bits.
 *
 * What d is: d = 1/2 dt (dt + dt_prev) u_tt + O(dt^3), with dt the step just
 * taken.  Times w/(1+w) it is the textbook local error of an implicit-Euler
 * step (theta = 1).  For the second-order steps (theta = 1/2, BDF2) it is a
 * conservative curvature control, NOT their O(dt^3) local error: that would
 * need a fourth time level, which is not kept.  c is the plain change of the
 * step.  What a controller does with the record is the caller's business.
 *
 * mgx_step_error(ctx, atol, rtol, out): MGX_E_ARG before any device call, with
 * a message that starts with the function's name, for a NULL argument, atol or
 * rtol not finite, negative or both zero, a context that is not at depth 2, and
 * a history without valid and valid2 (two steps since the last upload give
 * that; a rollback takes it away).  Single-GPU and local-parts contexts take it;
 * a local-parts context returns mgx_step_err_merge of its parts' owned-row
 * records in part order (of sub-context 0 when every level is replicated).  An
 * RCCL rank returns MGX_E_ARG -- the call communicates nothing -- and calls
 * mgx_step_error_rows (the owned rows of local part `part`; any context, a
 * single-GPU context has part 0) and merges.  u is read by the route
 * mgx_field_stats takes; pending and speculative state is left alone.
 * mgx_step_err_merge, host only: counts and sums add, the maxima by value,
 * err_max ties to the smaller (i, j); a record without a finite point leaves
 * the other's maxima alone; MGX_E_ARG (nothing changed) when the records' w
 * differ.
 * Raw op mgx_array_step_error: device pointers, reference layout, any n >= 2,
 * null stream; synchronises.  w finite.
 * Accounting: compulsory bytes 24 per interior point; the read-only tuning keys
 * "errest_us" / "errest_bytes" (mgx_get_tuning) give the device microseconds and
 * bytes of the calling thread's last call, as "stats_us" / "stats_bytes" do.
 * Measured at N=16384 on one MI355X: DESIGN.md section 14. */
typedef struct mgx_step_err {
    long   count;        /* interior points examined */
    long   nonfinite;    /* points whose e is NaN or +-Inf; excluded from everything below */
    double w;            /* dt_prev / dt_prev2, as used */
    double err_sum_sq, err_max;   /* e */
    long   err_max_i, err_max_j;
    double d_sum_sq, d_max;       /* d */
    double c_sum_sq, c_max;       /* c */
} mgx_step_err;
int mgx_set_history_depth(mgx_ctx *ctx, int depth);
int mgx_history_depth(mgx_ctx *ctx, int *depth, int *valid2, double *dt_prev2);
int mgx_step_error(mgx_ctx *ctx, double atol, double rtol, mgx_step_err *out);
int mgx_step_error_rows(mgx_ctx *ctx, int part, double atol, double rtol, mgx_step_err *out);
int mgx_step_err_merge(mgx_step_err *into, const mgx_step_err *other);
int mgx_array_step_error(const double *u, const double *h, const double *h2, long n, double w,
                         double atol, double rtol, mgx_step_err *out);

/* ---- Dense output: time-interpolated fields, samples and point probes ----------
 * An adaptive loop produces solutions at the times its controller chooses;
 * frames, coarse pictures and sensor readings are wanted at times the caller
 * chooses (the t_eval / dense_output of an ODE library).  After any step the
 * levels lie in HBM already -- u = u^(n+1), h = u^n and, at depth 2, h2 =
 * u^(n-1), with dt_prev and dt_prev2 known to the context -- and one pass
 * (csrc/dense.hip, part of mgx_build_sources_id) evaluates the interpolant
 * through them at a time inside the last step, without a download and without
 * clipping dt to land on the output time.
 *
 * Meaning, bit for bit.  tau = t* - t^(n+1) <= 0 is the offset of the output
 * time from the newest level; dt1 = dt_prev and dt2 = dt_prev2 as
 * mgx_history_info and mgx_history_depth report them.  All C doubles, every
 * operation rounded, nothing contracted, in either fp_mode.
 * mgx_dense_weights(order, tau, dt1, dt2, &w0, &w1, &w2), host only:
 *   order 0:  w0 = 1, w1 = w2 = 0
 *   order 1:  linear through u and h:  w1 = (0.0 - tau) / dt1, w0 = 1.0 - w1,
 *             w2 = 0; dt2 is ignored
 *   order 2:  the Lagrange quadratic on the nodes 0, -dt1, -(dt1+dt2): with
 *             s = dt1 + dt2, a = tau + dt1, b = tau + s
 *                 w0 = (a * b) / (dt1 * s)
 *                 w1 = ((0.0 - tau) * b) / (dt1 * dt2)
 *                 w2 = (tau * a) / (s * dt2)
 * MGX_E_ARG for an order outside 0..2, a non-finite tau, dt1 non-finite or not
 * positive at order >= 1, dt2 non-finite or not positive at order 2.  Any output
 * pointer may be NULL.  A tau outside [-dt1, 0] (order 2: [-(dt1+dt2), 0])
 * extrapolates; that is the caller's business and nothing is refused.
 * At a point
 *   order 0:  out = u, the same bits
 *   order 1:  out = fl( fl(w0*u) + fl(w1*h) )
 *   order 2:  out = fl( fl( fl(w0*u) + fl(w1*h) ) + fl(w2*h2) )
 * Order 1 does not read h2 and order 0 reads neither history array.  tau = 0
 * gives the weights (1, 0, 0) exactly at every order, so the output equals u by
 * value (the sign of a zero is not promised at order >= 1).
 *
 * Entry points.  All check their arguments and the context's state before any
 * device call and report MGX_E_ARG with a message that starts with the
 * function's own name.
 * mgx_dense_output(ctx, order, tau, stride, out) / mgx_dense_output_device:
 * out[a*(m+1)+b] = interpolant(a*stride, b*stride), m = N/stride -- the layout
 * and rules of mgx_sample / mgx_sample_device at level 0; stride divides N, and
 * stride 1 is the whole field in the reference layout, ring included.  The
 * host variant gathers into a compact device buffer and copies once.
 * mgx_dense_output_rows(ctx, part, order, tau, stride, out, &first_row, &rows):
 * the owned-rows form with the rules of mgx_sample_rows; any context (a
 * single-GPU context has part 0); out == NULL only reports first_row and rows.
 * mgx_dense_points(ctx, order, tau, npts, pi, pj, out): host index arrays and a
 * host out, out[k] = interpolant(pi[k], pj[k]), 0 <= pi, pj <= N; on an RCCL
 * rank every point must lie in the rank's owned rows; a bad index is MGX_E_ARG
 * and the message names k.  mgx_dense_points_device: device index arrays and a
 * device out; no host validation is possible, so the kernel writes NaN for an
 * index that is out of range or not held, and reads nothing for that entry.
 * npts = 0 is a no-op.  The index and value staging of the host form belongs to
 * the context, grows on demand and is freed by mgx_destroy.
 * Raw op mgx_array_dense(out, u, h, h2, n, w0, w1, w2, levels): device pointers,
 * reference layout, any n >= 1, null stream; synchronises.  levels (1 to 3) says
 * how many inputs are read -- the point formula of order levels - 1 with the
 * given weights; levels 1 copies u and reads no weight -- and the unused
 * pointers may be NULL.
 *
 * State.  Order >= 1 needs a history that is on and valid; order 2 needs depth
 * 2 with both valid and valid2.  Nothing else is checked: after a depth-2
 * rollback that kept valid, order 1 interpolates between u^(n-1) and u^n, which
 * is right.  u is read by the route mgx_field_stats takes (the level is
 * materialised, a packed pre-smoothed u expanded); pending and speculative
 * state is left alone, as the downloads leave it.  The weights use dt_prev and
 * dt_prev2, not the context's current dt: a mgx_set_time_step between the step
 * and the output call changes nothing.
 * Contexts, as mgx_sample*: single-GPU and local-parts contexts take the
 * whole-grid calls (each part writes its owned rows, sub-context 0 when every
 * level is replicated); an RCCL rank gets MGX_E_ARG from
 * mgx_dense_output[_device] and uses the rows form.  No call communicates.
 * Accounting: compulsory bytes 8 * (levels + 1) per output point (gathered
 * point at stride > 1), levels = order + 1; the read-only tuning keys
 * "dense_us" / "dense_bytes" (mgx_get_tuning) give the device microseconds and
 * bytes of the calling thread's last dense call, as "errest_us" /
 * "errest_bytes" do.  There is no profile kind for it.  Tuning keys of the
 * stride-1 pass (the same bits for every value): "dense_store" 0 (default) =
 * plain stores, 1 = non-temporal stores, 2 = one 16-byte store per column pair
 * on every row; "dense_rows" = the rows of a workgroup (default 4; 0 = the row
 * groups of the error pass).  Measured at N=16384 on one MI355X:
 * DESIGN.md section 15. */
int mgx_dense_weights(int order, double tau, double dt1, double dt2, double *w0, double *w1,
                      double *w2);
int mgx_dense_output(mgx_ctx *ctx, int order, double tau, long stride, double *out);
int mgx_dense_output_device(mgx_ctx *ctx, int order, double tau, long stride, double *out);
int mgx_dense_output_rows(mgx_ctx *ctx, int part, int order, double tau, long stride, double *out,
                          long *first_row, long *rows);
int mgx_dense_points(mgx_ctx *ctx, int order, double tau, long npts, const long *pi,
                     const long *pj, double *out);
int mgx_dense_points_device(mgx_ctx *ctx, int order, double tau, long npts, const long *pi,
                            const long *pj, double *out);
int mgx_array_dense(double *out, const double *u, const double *h, const double *h2, long n,
                    double w0, double w1, double w2, int levels);

/* ---- A predicted start for BDF2 steps from the resident history ----------------
 * After a step u^n, u^(n-1) and, at depth 2, u^(n-2) lie on the device, yet a
 * solve starts from u^n.  mgx_set_predictor(ctx, order) makes mgx_step_bdf2
 * form a guess g of u^(n+1) from them and start from whichever of u^n and g has
 * the smaller residual.  order 0 = off (the default), 1 = linear, 2 =
 * quadratic.  MGX_E_ARG before any device call, with a message that starts with
 * the function's name: a NULL ctx, an order outside 0..2, order > 0 on a
 * partitioned context (local parts and RCCL ranks alike: the guess would need a
 * ghost-row exchange).  Order 0 is accepted everywhere.  The call allocates
 * nothing, drops nothing and needs no history yet.  The setting belongs to the
 * context: it survives mgx_upload*, mgx_set_velocity*, mgx_set_source*,
 * mgx_set_time_step and mgx_rollback.  A context that never calls it launches
 * exactly what it launched before the predictor existed.
 * Only mgx_step_bdf2 changes, only while order > 0, and only on a step with no
 * ring pending from MGX_BC_NEXT_STEP: a step that takes a pending ring runs bit
 * for bit and launch for launch as with the predictor off.  mgx_step[_ex],
 * mgx_timestepper* and the raw ops are untouched.
 * The effective order e of a step is 2 when order 2 is set, the history is at
 * depth 2 and valid2 holds (mgx_history_depth), otherwise 1 -- a run that has
 * just started or has just been rolled back predicts linearly by itself.
 * The guess is the dense-output interpolant one step ahead: with (w0, w1, w2) =
 * mgx_dense_weights(e, tau = +dt, dt_prev, dt_prev2), dt the context's step and
 * dt_prev / dt_prev2 as they stand before the step, on rows and columns
 * 1..N-1
 *     e = 1:  g = fl( fl(w0 u) + fl(w1 h) )
 *     e = 2:  g = fl( fl( fl(w0 u) + fl(w1 h) ) + fl(w2 h2) )
 * (u = u^n, h = u^(n-1), h2 = u^(n-2); every operation rounded, none
 * contracted, in either fp_mode) and on the ring g = u, the same bits: what
 * mgx_array_dense computes.  At e = 1 it is also, bit for bit, the `up` that
 * mgx_step_error forms after the step, so the d of its record is then corrector
 * minus predictor.
 * The step: coefficients and right-hand side as without the predictor (rhs has
 * the same bits); r0 = |rhs - A u^n| and rp = |rhs - A g|, both in the
 * reference's term order with k = kA -- r0 is bit for bit the res0 the same
 * step returns with the predictor off; the history moves on as without it (h =
 * what mgx_download returned before the step, ring included; at depth 2 h2 =
 * the old h; valid flags and dt_prev values alike).  adopted = (rp < r0), false
 * when rp is NaN: u becomes g and the cycles start with res = rp; otherwise u
 * stays u^n and res = r0.  The loop is mg_outer's, while (iter < max_cycle &&
 * res / r0 > tol): the reference norm stays r0, the plain start's, so a
 * predicted step ends on the criterion a plain step ends on and zero cycles is
 * a legal outcome.  *res0 = r0; *res = the last norm, rp when no cycle ran.
 * MGX_E_NOCONV as without the predictor.
 * mgx_predictor_info: any pointer may be NULL.  order = the setting;
 * last_order = the effective order of the context's last mgx_step_bdf2, 0 if
 * none has run, the predictor was off or the step took a pending ring; adopted
 * = that step started from the guess; res_pred = rp, 0 when last_order is 0.
 * The pass (csrc/predict.hip, part of mgx_build_sources_id; profile kind
 * MGX_K_RHS) is one row march that forms rhs, g and both norms; it stores g
 * into a free finest-level buffer and no snapshot -- the history moves on by an
 * exchange of buffer pointers, one device copy more on a refused step.
 * Compulsory bytes per finest point: 8 * (3 + e) with velocity factors, + 16
 * without, + 8 with a field source; algorithmic bytes: those of the BDF2 pass +
 * 48 (the second residual) + 8 * (e + 2) (the guess).  Measured: DESIGN.md
 * section 16. */
int mgx_set_predictor(mgx_ctx *ctx, int order);
int mgx_predictor_info(mgx_ctx *ctx, int *order, int *last_order, int *adopted, double *res_pred);

#ifdef __cplusplus
}
#endif
#endif /* MGX_H */

// ctx.h -- internal: the solver context shared by mgx.hip (single GPU) and
// dist.hip (row-partitioned, multi-GPU).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mgx.h"
#include "boundary.h"
#include "dense.h"
#include "diag.h"
#include "kernels.h"

namespace mgxi {

int fail(int code, const std::string &msg);
int check_launch(const char *what);

#define HIPCHK(expr)                                                                     \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return ::mgxi::fail(MGX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define CHK(expr)              \
    do {                       \
        int rc_ = (expr);      \
        if (rc_) return rc_;   \
    } while (0)

struct Level {
    long n = 0, pitch = 0;
    double *u[3] = {nullptr, nullptr, nullptr};   // u[2]: finest level, cross-cycle pass
    int cur = 0;
    bool zero = false;   // u is logically all zeros (multigrid.cpp:77), not yet written
    // finest level only: index of the buffer holding the NEXT cycle's
    // pre-smoothed u (written by the cross-cycle pass, with rhs[1] restricted
    // from it and u[1] flagged zero), or -1
    int spec = -1;
    int xin = -1;   // finest level: the input buffer of the last cross-cycle pass
    // finest level: u[i] holds a packed u_pre (xsmooth.hip), which only the
    // cross pass reads; set on its u_pre buffer alone, so a buffer is packed
    // only while it is spec, xin or the input of the cycle under way
    bool packed[3] = {false, false, false};
    int nxt() const { return cur == 0 ? 1 : 0; }   // ping-pong partner of cur
    double *rhs = nullptr, *v1 = nullptr, *v2 = nullptr;
    // finest level: the next time step's rhs (step mode); coarsest level (n <=
    // 64, L >= 3): the rhs a W-cycle's fused pair pass restricts into while its
    // workgroups still read the current one for the fused coarsest solve
    double *rhs_alt = nullptr;
    // exact rank-1 factors of v1 / v2 (sepvel.h; row factors n+1, column
    // factors pitch, zero padded), or null: the passes that take them read
    // the 2-D v1 / v2 from HBM only where no factors exist
    double *sa1 = nullptr, *sb1 = nullptr, *sa2 = nullptr, *sb2 = nullptr;
    // rows >= vz of v1 and v2 are all zeros (found at upload): the row march
    // reads them from mgx_ctx::zrow (L2-resident) instead of HBM
    int vz = 0x7fffffff;
    // levels 1-2 of the reference tower, levels >= 1 of the correct one: v1 /
    // v2 equal the generator's entries from the finest factors (checked at
    // upload, stencil.h vg_col)
    bool vgen = false;
    // coef: the solve side A of the context's step (k = kA, mgx_ctx::kA), the
    // context's fp_mode; coef_rhs: what the compute_rhs kernels take, which
    // read the B side of a Coef alone (rr, nu, h, drhs) -- make_coef(kB) in the
    // bitwise form, or coef itself while kA == kB (Crank-Nicolson: every launch
    // gets the arguments it got before mgx_set_time_step existed)
    mgx::Coef coef{}, coef_rhs{};
    double M() const { return double(n + 1) * double(n + 1); }
    // compulsory bytes of v1 + v2 of this level (the zero rows cost no HBM)
    double Mv() const { return double(std::min<long>(n + 1, vz)) * double(n + 1); }
    double *U() const { return u[cur]; }
};

struct ProfRec {
    int kind, level;
    double bytes;    // canonical algorithmic bytes (SURVEY 8d per-op model)
    double cbytes;   // compulsory bytes: every array the launch reads or writes, once
    hipEvent_t e0, e1;
};

struct Dist;   // dist.hip

}  // namespace mgxi

struct mgx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    long N = 0;
    int L = 0;
    double dt = 0, nu = 0;
    // mgx_set_time_step: the theta-scheme (I + theta dt L) u' = (I - (1 - theta)
    // dt L) u + dt f is the reference's two operators with k = kA on the solve
    // side and k = kB on the right-hand side (C doubles, each product rounded:
    // every translation unit is built without contraction).  theta = 0.5 gives
    // kA == kB == dt exactly; two_op() is the schedules' branch test.
    double theta = 0.5;
    double kA() const { return (2.0 * theta) * dt; }
    double kB() const { return (2.0 * (1.0 - theta)) * dt; }
    bool two_op() const { return kA() != kB(); }
    // mgx_step_bdf2 (csrc/bdf.h): k_bdf != 0 = every level's coef is built with
    // that k instead of kA() (the BDF2 solve side, A = I + g dt L) until the next
    // mgx_rhs, mgx_step* or mgx_set_time_step puts the theta-scheme's back
    double k_bdf = 0;
    double k_solve() const { return k_bdf != 0 ? k_bdf : kA(); }
    // mgx_set_history: hist = one more finest-level array in the layout of
    // lv[0].u, u^n while u becomes u^(n+1) (a partitioned context keeps one in
    // every part, or in every sub-context where all levels are replicated, and
    // the flags here); hist_valid: it holds the u a step started from, and
    // hist_dt is that step's dt
    double *hist = nullptr;
    bool hist_on = false, hist_valid = false;
    double hist_dt = 0;
    // mgx_set_history_depth(ctx, 2): hist2 = a second array in the layout of
    // hist (in every part / sub-context as hist is; hist2_on here), u^(n-1)
    // after a step.  Every step stores its snapshot into the older buffer and
    // exchanges the two pointers; hist2_valid / hist2_dt are what hist_valid /
    // hist_dt were before the step.  hist_rolled: mgx_rollback has just moved
    // u^(n-1) into hist, so hist is no longer the u to go back to.
    double *hist2 = nullptr;
    bool hist2_on = false, hist2_valid = false, hist_rolled = false;
    double hist2_dt = 0;
    void hist_invalidate() { hist_valid = hist2_valid = hist_rolled = false; }
    // mgx_set_predictor (csrc/predict.h): pred_order = the setting (0 off); the
    // record of the last mgx_step_bdf2 -- pred_last its effective order (0: it
    // ran unpredicted), pred_adopted: it started from the guess, pred_res the
    // guess's residual norm
    int pred_order = 0, pred_last = 0;
    bool pred_adopted = false;
    double pred_res = 0;
    mgx_options opt{};
    std::vector<mgxi::Level> lv;
    double *partials = nullptr;   // norm partial sums
    double *dscal = nullptr;      // [0] norm, [2..3] coarse stats (iterations, last norm)
    double *hscal = nullptr;      // pinned host mirror
    double *stage[2] = {nullptr, nullptr};   // reference-layout (N+1)^2 staging
    double *zrow = nullptr;   // one row of zeros (finest pitch): Level::vz rows read it
    double2 *vga = nullptr;   // VGen::a of the Level::vgen levels, N+2 pairs
    // mgx_set_source: the context's own pitched copy of f (finest level, tower
    // layout), or null = the homogeneous equation; every finest compute_rhs
    // adds fl(fl(dt * src_scale) * f) through csrc/source.hip.  A partitioned
    // context keeps the copies in its parts (dist.hip) and src_active here.
    double *src = nullptr;
    double src_scale = 1.0;
    bool src_active = false;
    // mgx_set_source_separable: src_terms > 0 = the source is the sum of that
    // many outer products (source.h) and no copy of f exists.  src_a: the row
    // factors, MGX_SOURCE_MAX_TERMS x (N+1); src_b: the column factors,
    // MGX_SOURCE_MAX_TERMS x finest pitch, zero padded -- allocated by the first
    // call, reused by every replacement.  A partitioned context keeps the
    // factors in its parts (dist.hip) and src_terms here.
    int src_terms = 0;
    double *src_a = nullptr, *src_b = nullptr;
    bool has_source() const { return src != nullptr || src_terms > 0; }
    // scratch of the field diagnostics (diag.h: partial records + the result),
    // allocated by the first statistics call
    void *diag = nullptr;
    // staging of mgx_dense_points (csrc/dense.h): 2 * dense_cap indices (long)
    // followed by dense_cap values, grown on demand
    void *dense_buf = nullptr;
    long dense_cap = 0;
    // mgx_set_boundary: two rings of 4(N+1) doubles, allocated by the first
    // call that needs one -- [0] the pending ring of MGX_BC_NEXT_STEP
    // (bc_pending: the next mgx_step consumes it), [1] the staging of a host
    // ring written now and of mgx_get_boundary.  A partitioned context keeps
    // them here too: its parts and sub-contexts share the device and stream.
    double *bc_buf = nullptr;
    bool bc_pending = false;
    mgxbc::RingTimer bc_timer;   // tuning key "boundary_us"
    mgxi::Dist *dist = nullptr;   // row-partitioned multi-GPU state (dist.hip)
    // mg_outer's cycle predicted to be the last: its finest level runs the
    // post-smoothing alone, not the cross pass (no next-cycle pre-smoothing)
    bool post_only = false;
    // inside mgx_run_cycles: every cycle ends in a cross pass, so a packed
    // u_pre is never expanded (mg_outer's last cycle would have to: "xpack" 2)
    bool fixed_cycles = false;
    // the coarsest solve of level cf_level (cf_reps solves) deferred into the
    // prolongation tile pass of the level above (tuning key "coarse_fuse");
    // -1: none pending
    int cf_level = -1, cf_reps = 0;
    // time-step mode: inside mgx_step (step_next) the last cycle's cross pass
    // also forms the next step's rhs (lv[0].rhs_alt), initial norm
    // (step_res0) and first pre-smoothing + restriction (lv[0].spec, lv[1]
    // rhs); step_spec = that state is ready for the next mgx_step
    bool step_next = false, step_spec = false;
    bool no_rhs_alt = false;   // the step-mode rhs did not fit in HBM: plain schedule
    // tuning key "graph_level": the sub-cycle below a level replayed as a
    // captured hipGraph, one per entry state (mgx.hip graph_vcycle)
    struct Graph {
        std::vector<long> key, end;
        hipGraphExec_t exec = nullptr;
    };
    std::vector<Graph> graphs;
    bool capturing = false;
    double step_res0 = 0;
    // profiling
    int prof = 0;   // 0 off, 1 every launch, 2 finest-level launches only
    std::vector<mgxi::ProfRec> pending;
    std::vector<hipEvent_t> pool;
    double sum_ms[MGX_K_COUNT][64] = {};
    double sum_bytes[MGX_K_COUNT][64] = {};
    double sum_cbytes[MGX_K_COUNT][64] = {};
    long count[MGX_K_COUNT][64] = {};
};

namespace mgxi {

hipEvent_t take_event(mgx_ctx *c);

// A launch whose lambda declined (launched nothing: the caller saw a negative
// block count) drops the record it pushed, so profiles count real launches.
inline void unlaunch(mgx_ctx *c, size_t pending_before) {
    while (c->pending.size() > pending_before) {
        c->pool.push_back(c->pending.back().e0);
        c->pool.push_back(c->pending.back().e1);
        c->pending.pop_back();
    }
}
// Launch helper: records HIP events around the launch when profiling is on.
// bytes: canonical algorithmic bytes of the reference ops the launch does
// (SURVEY 8d); cbytes: its compulsory bytes (each array it must read or write,
// once) -- the roofline denominator of a fused pass.
template <class F>
int launch(mgx_ctx *c, int kind, int level, double bytes, double cbytes, F &&f) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool rec = c->prof == 1 || (c->prof == 2 && level == 0);
    if (rec) {
        e0 = take_event(c);
        e1 = take_event(c);
        if (e0) (void)hipEventRecord(e0, c->stream);
    }
    f();
    CHK(check_launch("kernel launch"));
    if (rec && e0 && e1) {
        (void)hipEventRecord(e1, c->stream);
        c->pending.push_back({kind, level, bytes, cbytes, e0, e1});
    }
    return MGX_OK;
}
// single-op launches: canonical == compulsory
template <class F>
int launch(mgx_ctx *c, int kind, int level, double bytes, F &&f) {
    return launch(c, kind, level, bytes, bytes, static_cast<F &&>(f));
}

int prof_flush(mgx_ctx *c);
int materialize(mgx_ctx *c, int l);
int op_expand(mgx_ctx *c);   // level 0's current buffer in full form (a packed u_pre)
int read_norm(mgx_ctx *c, double *norm);
// store_post: see op_cross (false only between cycles of one run_cycles call)
int op_vcycle(mgx_ctx *c, int l, double *norm = nullptr, bool store_post = true);
int op_rhs(mgx_ctx *c);
int op_residual_norm(mgx_ctx *c, int l, double *norm, double bytes_per_pt = 48.0);
int build_tower(mgx_ctx *c);
// Level::vz of levels 1..L-1 from the built tower (the first row from which
// every row of v1 and v2 is zero)
int find_zero_rows(mgx_ctx *c);
// velocity factors of level 0 from host copies of v1 / v2 (rows [r0, r0+rows)
// of width n+1); false: not separable (or "sep_velocity" off), nothing set
bool factor_velocity(const double *v1, const double *v2, long n, long r0, long rows, double smin,
                     std::vector<double> &a1, std::vector<double> &b1, std::vector<double> &a2,
                     std::vector<double> &b2, long *js1 = nullptr, long *js2 = nullptr);
int set_level_factors(Level &L, long row0, const std::vector<double> &a1,
                      const std::vector<double> &b1, const std::vector<double> &a2,
                      const std::vector<double> &b2, hipStream_t s);
void free_level_factors(Level &L);
extern long g_sep_velocity;
extern long g_vgen;   // tuning key "vgen" (mgx.hip)
void free_ctx(mgx_ctx *c);
// Create a single-GPU context; stream != nullptr: borrow that stream.
int create_ctx(mgx_ctx **out, long n, int maxlvl, double dt, double nu, const mgx_options *opt,
               hipStream_t stream);
int upload_ctx(mgx_ctx *c, const double *u0, const double *v1, const double *v2,
               hipMemcpyKind kind);
// mgx_set_source on a single-GPU context (f == nullptr removes it); every
// state formed from the old right-hand side is dropped
int set_source_ctx(mgx_ctx *c, const double *f, hipMemcpyKind kind);
void drop_source_state(mgx_ctx *c);
// mgx_set_source_separable on a single-GPU context: a, b hold terms x (N+1)
// doubles, term-major (checked by the caller); replaces a field source
int set_source_sep_ctx(mgx_ctx *c, int terms, const double *a, const double *b,
                       hipMemcpyKind kind);
// the device copies of separable factors (ctx.h mgx_ctx::src_a / src_b layout
// for a level of n+1 columns and the given pitch), allocated where *da / *db
// are null; who: the C entry point, for the message
int copy_source_factors(double **da, double **db, long n, long pitch, int terms, const double *a,
                        const double *b, hipMemcpyKind kind, hipStream_t s, const char *who);
// mgx_set_time_step on one context's own state (mgx.hip): dt, theta, every
// level's coef / coef_rhs, and everything formed with the old coefficients
// dropped -- drop_source_state's list, a deferred coarsest solve, the captured
// sub-cycles (they hold Coef as kernel arguments).  The caller has expanded a
// packed u_pre (op_expand, with the old coefficients) where one can exist.
// k_bdf: mgx_ctx::k_bdf from the call on (0: the theta-scheme's solve side)
int retime_ctx(mgx_ctx *c, double dt, double theta, double k_bdf = 0.0);
// the two Coefs of a level of spacing h for the context's dt and theta
void step_coefs(const mgx_ctx *c, double h, mgx::Coef *coef, mgx::Coef *coef_rhs);
// ... and on a partitioned context (dist.hip): every part's PLevel and every
// replicated sub-context; no communication
int dist_set_time_step(mgx_ctx *c, double dt, double theta, double k_bdf = 0.0);
// mgx_set_history and what goes with it (csrc/bdf.h) on one context's own
// state (mgx.hip).  hist_alloc_ctx: MGX_E_HIP with a message when there is no
// room; hist_snapshot_ctx: hist = what mgx_download would return now;
// op_rhs_norm_bdf: the BDF2 pass (rhs, h <- u, the norm against coef) with the
// source weight cf; hist_restore_ctx: u = hist, everything formed with the old
// u dropped (boundary_prepare_ctx).  None synchronises but the norm read.
int hist_alloc_ctx(mgx_ctx *c, const char *who);
void hist_free_ctx(mgx_ctx *c);
int hist_snapshot_ctx(mgx_ctx *c);
int op_rhs_norm_bdf(mgx_ctx *c, double b0, double b1, double cf, double *res0);
// the same pass with a predicted start (csrc/predict.h; single-GPU contexts):
// rhs, the guess of effective order e (weights w) into level 0's free buffer,
// *res0 = |rhs - A u|, *resp = |rhs - A g|.  Stores no snapshot: the caller
// moves the history on by exchanging pointers (mgx_step_bdf2).
int op_predict_bdf(mgx_ctx *c, double b0, double b1, double cf, int e, const double w[3],
                   double *res0, double *resp);
int hist_restore_ctx(mgx_ctx *c);
// ... and on a partitioned context (dist.hip): every part's owned rows, or
// every sub-context where all levels are replicated.  dist_rhs_norm_bdf mirrors
// dist_rhs_norm's two-operator branch: the u ghosts before, the rhs ghosts after
int dist_set_history(mgx_ctx *c, int on, const char *who);
// mgx_set_history_depth (1 <-> 2) on one context's own state: hist2 allocated
// and zeroed (hist too while it holds nothing valid: a pass stores whole column
// pairs up to column n, the pad columns behind them must stay zeros), or freed
int hist2_alloc_ctx(mgx_ctx *c, bool zero_hist, const char *who);
void hist2_free_ctx(mgx_ctx *c);
// ... and on every part or sub-context (all or none); zero_hist as above
int dist_set_history2(mgx_ctx *c, int on, bool zero_hist, const char *who);
// depth 2, before a step's snapshot or BDF2 pass: hist <-> hist2 in the context
// (every part / sub-context), so that the pass writes the older buffer
void hist_swap(mgx_ctx *c);
void dist_hist_swap(mgx_ctx *c);
// mgx_step_error[_rows] (csrc/errest.h; mgx.hip): the record of interior rows
// of [r0, r1) of three arrays in one tower layout, on c's stream and
// diagnostics scratch.  Synchronises the stream.
int step_error_view(mgx_ctx *c, const double *u, const double *h, const double *h2, long row0,
                    long pitch, long n, long r0, long r1, double w, double atol, double rtol,
                    mgx_step_err *out);
// ... on a partitioned context (dist.hip): the owned rows of one local part,
// and the merge of the parts' records in part order (local parts only)
int dist_step_error_rows(mgx_ctx *c, int part, double w, double atol, double rtol,
                         mgx_step_err *out, const char *who);
int dist_step_error(mgx_ctx *c, double w, double atol, double rtol, mgx_step_err *out);
// tuning key "dense_store" (mgx.hip): how the dense march stores out (dense.h)
extern long g_dense_store;
extern long g_dense_rows;   // tuning key "dense_rows"
// Dense output (csrc/dense.h; mgx.hip), shared with dist.hip.  A piece: the
// arrays of one part (Src with the weights set) and the sampled rows A in [A0,
// A1) it writes (fine rows A * stride; stride 1: the rows themselves).
struct DensePiece {
    mgxdense::Src s;
    long A0 = 0, A1 = 0;
};
// out[(A - A0) * (n/stride + 1) + B] for the pieces' rows, `rows` rows in all:
// the march (stride 1) or the gather into a compact device buffer that is
// copied once (host out), or into out itself (device out).  Synchronises.
int dense_pieces(mgx_ctx *c, const std::vector<DensePiece> &pieces, long stride, long A0,
                 long rows, double *out, bool device_out);
// A piece of the point probes: the rows [A0, A1) are the rows the arrays hold
// and answer for.  pi, pj, out: device; fill_unheld: a valid point in no piece's
// rows gives NaN.  Synchronises.
int dense_points_pieces(mgx_ctx *c, const std::vector<DensePiece> &pieces, bool fill_unheld,
                        long npts, const long *pi, const long *pj, double *out);
// the single-GPU context's arrays (u by field_view's route) with the weights w
int dense_src_ctx(mgx_ctx *c, int levels, const double w[3], mgxdense::Src *s);
// ... on a partitioned context (dist.hip); `who` names the C entry point
int dist_dense(mgx_ctx *c, int levels, const double w[3], long stride, double *out,
               bool device_out, const char *who);
int dist_dense_rows(mgx_ctx *c, int part, int levels, const double w[3], long stride, double *out,
                    long *first_row, long *rows, const char *who);
// the points of every local part's owned rows (of sub-context 0 where every
// level is replicated); device pointers.  An RCCL rank's other rows give NaN.
int dist_dense_points(mgx_ctx *c, int levels, const double w[3], long npts, const long *pi,
                      const long *pj, double *out);
int dist_snapshot(mgx_ctx *c);
int dist_rhs_norm_bdf(mgx_ctx *c, double b0, double b1, double cf, double *res0);
int dist_rollback(mgx_ctx *c);
// tuning key "source_sv" (mgx.hip): the source pass reads the finest level's
// velocity factors, where the context keeps them, instead of the 2-D v1 / v2
extern long g_source_sv;

// mgx_set_boundary(MGX_BC_NOW) on a single-GPU context (mgx.hip; csrc/
// boundary.hip).  boundary_prepare_ctx: the finest u in full form in its
// current buffer, and everything formed with the old ring dropped;
// boundary_scatter_ctx: the ring g (device) into that buffer on c's stream.
// Neither synchronises.
int boundary_prepare_ctx(mgx_ctx *c);
int boundary_scatter_ctx(mgx_ctx *c, const double *g);
// ... and on a partitioned context (dist.hip): every part's allocated rows, or
// every sub-context where all levels are replicated; timed by c->bc_timer
int dist_boundary_now(mgx_ctx *c, const double *g);
// mgx_get_boundary of a local-parts context: each part's owned rows into g
// (device); an RCCL rank: MGX_E_ARG (who: the C entry point, for the message),
// checked before any device call
int dist_boundary_gather(mgx_ctx *c, double *g, const char *who);

// Field diagnostics (mgx.hip; csrc/diag.hip), shared with dist.hip.
// The statistics of rows [r0, r1) of a field on c's stream and scratch;
// interior: rows and columns 1..n-1 only; minus (reference layout, or null)
// holds rows from minus_row0 on.  Synchronises the stream.
int stats_view(mgx_ctx *c, const mgxdiag::View &f, long r0, long r1, int interior,
               const double *minus, long minus_row0, mgx_stats *out);
// sampled rows A in [A0, A1) (fine rows A * stride) of a field
struct SamplePiece {
    mgxdiag::View f;
    long A0 = 0, A1 = 0;
};
// out[(A - A0) * (n/stride + 1) + B] for the pieces' rows, `rows` rows in all:
// gathered into a compact device buffer and copied (host out), or written by
// the kernel (device out).  Synchronises the stream.
int sample_pieces(mgx_ctx *c, const std::vector<SamplePiece> &pieces, long stride, long A0,
                  long rows, double *out, bool device_out);
// the field mgx_download_level(level, field) copies (4 = the source copy, 5 / 6
// = the history arrays hist / hist2) of a single-GPU context
int field_view(mgx_ctx *c, int level, int field, mgxdiag::View *v);
// fields 5 / 6 = the history arrays hist / hist2 (level 0): MGX_E_ARG where the
// array is absent or not valid by c's flags; host only
int history_field_check(const mgx_ctx *c, int level, int field, const char *who);

// dist.hip entry points used by the C ABI
int dist_upload(mgx_ctx *c, const double *u0, const double *v1, const double *v2,
                hipMemcpyKind kind);
int dist_download(mgx_ctx *c, double *u, hipMemcpyKind kind);
int dist_owned_rows(mgx_ctx *c, int part, int *ra, int *rb);
int dist_download_rows(mgx_ctx *c, int part, double *out, hipMemcpyKind kind);
// field diagnostics of a partitioned context (level 0; `who` names the C entry
// point in messages): the owned rows of one local part, minus_rows holding
// rows from minus_row0 on (the part's first owned row when < 0) ...
int dist_field_stats_rows(mgx_ctx *c, int part, int field, int interior, const double *minus,
                          long minus_row0, mgx_stats *out, const char *who);
// ... and the whole grid of a local-parts context: the parts' records merged
// in part order
int dist_field_stats(mgx_ctx *c, int level, int field, int interior, const double *minus,
                     mgx_stats *out);
int dist_sample(mgx_ctx *c, int level, int field, long stride, double *out, bool device_out,
                const char *who);
int dist_sample_rows(mgx_ctx *c, int part, int field, long stride, double *out, long *first_row,
                     long *rows);
int dist_rhs(mgx_ctx *c);
int dist_rhs_norm(mgx_ctx *c, double *res0);
// whole-grid source (reference layout): every part keeps its owned rows, the
// replicated sub-contexts of a fully replicated context the whole field
int dist_set_source(mgx_ctx *c, const double *f, hipMemcpyKind kind);
// mgx_set_source_rows: f[i] = the owned rows of local part i (null entries
// refused by the caller)
int dist_set_source_rows(mgx_ctx *c, const double *const *f, hipMemcpyKind kind);
// mgx_set_source_separable: every part (or replicated sub-context) keeps the
// factors
int dist_set_source_sep(mgx_ctx *c, int terms, const double *a, const double *b,
                        hipMemcpyKind kind);
void dist_set_source_scale(mgx_ctx *c, double s);
int dist_vcycle(mgx_ctx *c, double *norm, bool store_post = true);
// partitioned level 0 runs the cross-cycle pass; recompute its unstored u_post
bool dist_post_predictable(mgx_ctx *c);
int dist_redo_post(mgx_ctx *c);
int dist_residual_norm(mgx_ctx *c, double *norm);
void dist_free(mgx_ctx *c);
// replicated coarse-level contexts of a partitioned context (one per local part)
int dist_nsub(mgx_ctx *c);
mgx_ctx *dist_sub(mgx_ctx *c, int i);
int dist_la(mgx_ctx *c);
int dist_velocity_mask(mgx_ctx *c);   // mgx_velocity_factored of a partitioned context
int dist_settle(mgx_ctx *c);   // join the side stream's exchanges into the compute stream
// levels whose row blocks would be shorter than this are replicated (tuning
// key "dist_min_rows", default 256)
extern long g_dist_min_rows;
// tuning key "dist_overlap" (dist.hip): finest-level ghost exchange on a second
// stream beside the interior of the cross-cycle pass
extern long g_dist_overlap;
// tuning key "dist_local_side" (dist.hip): virtual ranks' early exchanges on
// the compute stream (0) or the second stream (1)
extern long g_dist_local_side;
extern long g_dist_comm_chain;   // tuning key "dist_comm_chain" (test hook)
// tuning key "cross_cycle" (mgx.hip); levels with n >= kCrossMinN can use it
bool cross_cycle_on();
constexpr long kCrossMinN = 4096;

}  // namespace mgxi

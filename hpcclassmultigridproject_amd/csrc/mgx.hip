// mgx.hip -- context, V-cycle orchestration and the C ABI of include/mgx.h.
//
// Host control flow mirrors the reference solver (multigrid.cpp:17-186) call
// for call; every stencil op is a CDNA4 kernel from kernels.hip on the
// context's stream.  The level towers live in HBM in the "tower layout"
// (row pitch round_up(n+1,16) doubles); u has two buffers per level because
// the one-pass smoother is out of place (ping-pong).  Row-partitioned
// multi-GPU contexts (ctx->dist) are implemented in dist.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ctx.h"
#include "diag.h"
#include "sepvel.h"
#include "source.h"
#include "tstep.h"
#include "bdf.h"
#include "errest.h"
#include "dense.h"
#include "predict.h"
#include "vfactor.h"

namespace mgxi {

thread_local std::string g_err;

// tuning key "sep_velocity": 1 (default) = at upload, a velocity field that is
// an exact rank-1 outer product (the reference's rotating flow) is also kept
// as its factors and the finest-level cross pass reads those instead of the
// 2-D v1 / v2 (sepvel.h; bitwise the same results); 0 = always the 2-D arrays
long g_sep_velocity = 1;

bool factor_velocity(const double *v1, const double *v2, long n, long r0, long rows, double smin,
                     std::vector<double> &a1, std::vector<double> &b1, std::vector<double> &a2,
                     std::vector<double> &b2, long *js1, long *js2) {
    (void)r0;
    if (!g_sep_velocity || !v1 || !v2 || rows < 1) return false;
    const long w = n + 1;
    a1.assign(rows, 0.0);
    a2.assign(rows, 0.0);
    b1.assign(w, 0.0);
    b2.assign(w, 0.0);
    return mgxsep::factor_rank1(v1, rows, w, w, smin, a1.data(), b1.data(), 0, js1) &&
           mgxsep::factor_rank1(v2, rows, w, w, smin, a2.data(), b2.data(), 0, js2);
}

// tuning key "device_factor": which uploads factor the velocity with the device
// backend (vfactor.hip) on the finest level's tower copy: 1 (default) = those
// from device pointers (the host never sees their fields), 2 = those from host
// pointers too (after their copy), 0 = none: a device upload keeps the 2-D
// arrays.  The same factors either way (sepvel.h decides for both backends).
long g_device_factor = 1;

// factor_velocity on the context's own copy of the finest v1 / v2; *found =
// both fields are rank-1
static int factor_velocity_device(mgx_ctx *c, double smin, std::vector<double> &a1,
                                  std::vector<double> &b1, std::vector<double> &a2,
                                  std::vector<double> &b2, bool *found) {
    *found = false;
    const Level &L = c->lv[0];
    const long w = c->N + 1;
    a1.assign(w, 0.0);
    a2.assign(w, 0.0);
    b1.assign(w, 0.0);
    b2.assign(w, 0.0);
    if (!g_sep_velocity) return MGX_OK;
    for (int f = 0; f < 2; ++f) {
        hipError_t e = hipSuccess;
        const int r = mgxvf::factor_rank1_device(f ? L.v2 : L.v1, w, w, L.pitch, smin,
                                                 (f ? a2 : a1).data(), (f ? b2 : b1).data(),
                                                 c->stream, nullptr, &e);
        if (r < 0)
            return fail(MGX_E_HIP, std::string("device velocity factorisation: ") +
                                       hipGetErrorString(e));
        if (r == 0) return MGX_OK;
    }
    *found = true;
    return MGX_OK;
}

void free_level_factors(Level &L) {
    for (double **p : {&L.sa1, &L.sb1, &L.sa2, &L.sb2}) {
        (void)hipFree(*p);
        *p = nullptr;
    }
}

// Device copies: row factors at rows [row0, row0 + a.size()) of an (n+1)-row
// array (the rest zero), column factors zero padded to the pitch.
int set_level_factors(Level &L, long row0, const std::vector<double> &a1,
                      const std::vector<double> &b1, const std::vector<double> &a2,
                      const std::vector<double> &b2, hipStream_t s) {
    free_level_factors(L);
    const size_t ra = sizeof(double) * (size_t)(L.n + 1), rb = sizeof(double) * (size_t)L.pitch;
    HIPCHK(hipMalloc(&L.sa1, ra));
    HIPCHK(hipMalloc(&L.sa2, ra));
    HIPCHK(hipMalloc(&L.sb1, rb));
    HIPCHK(hipMalloc(&L.sb2, rb));
    for (double *p : {L.sa1, L.sa2}) HIPCHK(hipMemsetAsync(p, 0, ra, s));
    for (double *p : {L.sb1, L.sb2}) HIPCHK(hipMemsetAsync(p, 0, rb, s));
    HIPCHK(hipMemcpyAsync(L.sa1 + row0, a1.data(), sizeof(double) * a1.size(),
                          hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(L.sa2 + row0, a2.data(), sizeof(double) * a2.size(),
                          hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(L.sb1, b1.data(), sizeof(double) * b1.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(L.sb2, b2.data(), sizeof(double) * b2.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // the host vectors may go out of scope
    return MGX_OK;
}

// Cross-cycle fusion of the finest level (k_xsmooth) on levels this large
// (the row-march regime); tuning key "cross_cycle" turns it off.
long g_cross_cycle = 1;
bool cross_cycle_on() { return g_cross_cycle != 0; }

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

int check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MGX_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return MGX_OK;
}

hipEvent_t take_event(mgx_ctx *c) {
    if (!c->pool.empty()) {
        hipEvent_t e = c->pool.back();
        c->pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

int prof_flush(mgx_ctx *c) {
    if (c->pending.empty()) return MGX_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto &r : c->pending) {
        float ms = 0.f;
        // (a partitioned context times its side-stream exchanges too)
        HIPCHK(hipEventSynchronize(r.e1));
        HIPCHK(hipEventElapsedTime(&ms, r.e0, r.e1));
        int lvl = r.level < 0 ? 0 : (r.level > 63 ? 63 : r.level);
        c->sum_ms[r.kind][lvl] += ms;
        c->sum_bytes[r.kind][lvl] += r.bytes;
        c->sum_cbytes[r.kind][lvl] += r.cbytes;
        c->count[r.kind][lvl] += 1;
        c->pool.push_back(r.e0);
        c->pool.push_back(r.e1);
    }
    c->pending.clear();
    return MGX_OK;
}

// ---------------------------------------------------------------- level ops
static int op_wexpand(mgx_ctx *c, int l);
int materialize(mgx_ctx *c, int l) {
    Level &L = c->lv[l];
    if (!L.zero) return op_wexpand(c, l);   // (whole rows for whoever reads them)
    HIPCHK(hipMemsetAsync(L.U(), 0, sizeof(double) * L.pitch * (L.n + 1), c->stream));
    L.zero = false;
    if (l >= 1) L.packed[L.cur] = false;
    return MGX_OK;
}

// `sweeps` RB-GS sweeps (gauss_seidel, gs.cpp:109) on level l.
//   prolong:  first apply u[l] += P(u[l+1]) (multigrid.cpp:81-83);
//   restrict: afterwards restrict the residual into rhs[l+1] (multigrid.cpp:73-75);
//   norm:     afterwards compute the residual norm into c->dscal[0].
// With the temporally blocked smoother all three are fused into the first /
// last smoothing pass; *fused_norm tells the caller whether the norm was done.
int op_prolong_add(mgx_ctx *c, int l);
int op_restrict(mgx_ctx *c, int l);
// tuning key "vgen": 1 (default) = levels 1-2 of the reference tower and
// every coarse level of the correct tower, when their velocity passed the
// upload check (find_vgen), generate v1 / v2 in the V-cycle's 3-sweep passes
// from the finest factors instead of reading them (stencil.h vg_col; bitwise
// the same); 0 = reads them
long g_vgen = 1;
static mgx::VGen level_vgen(const mgx_ctx *c, int l) {
    mgx::VGen g;
    g.a = c->vga;
    g.b1 = c->lv[0].sb1;
    g.b2 = c->lv[0].sb2;
    g.l = l;
    g.strided = c->opt.tower_mode == MGX_TOWER_CORRECT ? 1 : 0;
    return g;
}
// tuning key "coarse_fuse": 1 (default) = the coarsest solve (n <= 64, u in
// LDS) runs inside the prolongation tile pass of the level above: every
// workgroup of that pass solves the coarsest level in its LDS and prolongs
// from the copy (mgx::CoarseFuse), one launch less per visit -- bitwise the
// same; 0 = its own launch (op_coarse)
long g_coarse_fuse = 1;
int op_coarse(mgx_ctx *c, int l, int reps);
// (only from a zero start, the V- and W-cycle's case after the restriction:
// then no workgroup reads the coarse u that workgroup 0 stores at its end;
// and only with nsmooth >= 1, so that the post-smoothing above is a tile pass
// that can take it -- nsmooth 0 prolongs with op_prolong_add)
static bool coarse_fusable(const mgx_ctx *c, int l) {
    return g_coarse_fuse && !c->dist && c->opt.smoother == 0 && c->opt.nsmooth >= 1 &&
           l == c->L - 1 && l >= 2 && c->lv[l].zero &&
           c->lv[l].n <= mgx::kCoarseLdsMaxN && mgx::get_coarse_lds() &&
           c->lv[l - 1].n <= mgx::get_tile_max_n();
}
// run a pending fused coarsest solve on its own (its consumer cannot take it)
static int flush_coarse(mgx_ctx *c) {
    if (c->cf_level < 0) return MGX_OK;
    const int l = c->cf_level;
    c->cf_level = -1;
    return op_coarse(c, l, c->cf_reps);
}
// A pass that restricts into the rhs its fused coarsest solve reads would race
// (every workgroup loads cf.rhs at its start while others already store the
// restriction): refuse it.  mode: the pass's kMode bits.
static int check_coarse_rhs(const mgx::SmoothArgs &A, int mode) {
    if (A.cf.on && (mode & mgx::kModeRestrict) && A.rhsc == A.cf.rhs)
        return fail(MGX_E_INTERNAL, "fused coarsest solve reads the rhs its pass restricts into");
    return MGX_OK;
}
// the pending coarsest solve of level l+1 into a prolongation pass of level l
static bool take_coarse(mgx_ctx *c, int l, mgx::SmoothArgs &A) {
    if (c->cf_level != l + 1) return false;
    Level &Cl = c->lv[l + 1];
    A.cf.u = Cl.U();
    A.cf.rhs = Cl.rhs;
    A.cf.v1 = Cl.v1;
    A.cf.v2 = Cl.v2;
    A.cf.n = Cl.n;
    A.cf.pitch = Cl.pitch;
    A.cf.c = Cl.coef;
    A.cf.tol = c->opt.coarse_tol;
    A.cf.maxit = c->opt.coarse_maxit;
    A.cf.zero_first = Cl.zero ? 1 : 0;
    A.cf.reps = c->cf_reps;
    A.cf.stats = c->dscal + 2;
    A.cf.on = 1;
    return true;
}
// after a launch that took it: the coarse level holds its solution
static void took_coarse(mgx_ctx *c, int l) {
    c->cf_level = -1;
    c->lv[l + 1].zero = false;
}

// tuning key "wpack": levels >= 1, whose pre- and post-smoothing are wave
// marches, pass the pre-smoothed u between the two as one colour (wsmooth.hip
// PK): 0 whole rows, 1 packed wherever that form exists, 2 packed in fp_mode
// fma only.  Level::packed[i] of a level >= 1 marks u[i] as such a buffer; it
// is set by the pre-smoothing of op_vcycle alone (pack_out) and consumed by
// the same call's post-smoothing; any other reader gets whole rows first
// (op_wexpand).  3 (test hook): packed as 1, and every post-smoothing takes
// the expansion path.  Default 2 -- measured at N=16384, L=9, alternated in
// one process: fma level 1 0.610-0.613 -> 0.550-0.555 ms and the V-cycle 2.42-
// 2.55 -> 2.34-2.35 ms; bitwise (division bound) level 1 0.721-0.723 -> 0.715-
// 0.721 ms, inside the spread.
long g_wpack = 2;
static bool wpack_on(const Level &L) {
    return g_wpack == 1 || g_wpack == 3 || (g_wpack == 2 && L.coef.fm);
}

// Whole rows in place of level l's packed pre-smoothed u: the pre-smoothing
// (from zero, without its restriction) once more into the same buffer -- the
// colour that was dropped cannot be rebuilt from the kept one, and no default
// path comes here (a post-smoothing that turned out not to be a packed march)
static int op_wexpand(mgx_ctx *c, int l) {
    Level &L = c->lv[l];
    if (l < 1 || !L.packed[L.cur]) return MGX_OK;
    const int k = c->opt.nsmooth;
    mgx::SmoothArgs A{};
    A.uin = L.u[L.cur];
    A.uout = L.u[L.cur];
    A.rhs = L.rhs;
    A.v1 = L.v1;
    A.v2 = L.v2;
    A.zrow = c->zrow;
    A.vz = L.vz;
    A.n = L.n;
    A.pitch = L.pitch;
    A.c = L.coef;
    A.partials = c->partials;
    A.norm_out = c->dscal;
    int blocks = 0;
    CHK(launch(c, MGX_K_GS, l, 40.0 * k * L.M(), 8.0 * (2.0 * L.M() + 2.0 * L.Mv()),
               [&] { blocks = mgx::launch_smooth(A, k, mgx::kModeZero, c->stream); }));
    if (blocks < 0) return fail(MGX_E_INTERNAL, "op_wexpand: unsupported sweeps");
    L.packed[L.cur] = false;
    return MGX_OK;
}

int op_smooth(mgx_ctx *c, int l, int sweeps, bool prolong, bool restrict_, bool norm,
              bool *fused_norm, bool pack_out = false) {
    Level &L = c->lv[l];
    if (fused_norm) *fused_norm = false;
    if (c->opt.smoother != 0 || sweeps <= 0) CHK(op_wexpand(c, l));   // (whole rows below)
    if (c->opt.smoother == 0 && sweeps > 0) {
        const int fuse = std::max(1, std::min(c->opt.fuse, mgx::kSmoothMaxSweeps));
        int done = 0;
        while (done < sweeps) {
            const int k = std::min(sweeps - done, fuse);
            const bool first = done == 0, last = done + k == sweeps;
            const bool pr = prolong && first && !L.zero;
            const bool rs = restrict_ && last;
            const bool nm = norm && last && !rs;
            // a pending coarsest solve of level l+1 runs inside this pass
            // (its u is then not read from HBM: no zero fill either)
            const bool cfuse = pr && c->cf_level == l + 1;
            if (pr && !cfuse) CHK(materialize(c, l + 1));
            int mode = 0;
            if (L.zero) mode |= mgx::kModeZero;
            if (pr) mode |= mgx::kModeProlong;
            if (rs) mode |= mgx::kModeRestrict;
            if (nm) mode |= mgx::kModeNorm;
            mgx::SmoothArgs A{};
            A.uin = L.u[L.cur];
            A.uout = L.u[L.nxt()];
            A.rhs = L.rhs;
            A.v1 = L.v1;
            A.v2 = L.v2;
            A.zrow = c->zrow;
            A.vz = L.vz;
            if (L.vgen && g_vgen) A.vg = level_vgen(c, l);
            A.n = L.n;
            A.pitch = L.pitch;
            A.c = L.coef;
            if (pr || rs) {
                Level &Cl = c->lv[l + 1];
                A.uc = Cl.U();
                A.rhsc = Cl.rhs;
                A.pitchc = Cl.pitch;
            }
            A.partials = c->partials;
            A.norm_out = c->dscal;
            if (cfuse) take_coarse(c, l, A);
            // (wpack: both passes of the level must be marches; a packed input
            // whose pass is none after all is expanded in place first)
            const bool pk_form = l >= 1 && !c->dist && first && last && (k == 2 || k == 3) &&
                                 mgx::smooth_packs(A, k);
            if (l >= 1 && L.packed[L.cur] &&
                (!(pk_form && mode == mgx::kModeProlong) || g_wpack == 3))
                CHK(op_wexpand(c, l));
            A.pin = l >= 1 && L.packed[L.cur];
            A.pout = pack_out && pk_form && wpack_on(L) &&
                     mode == (mgx::kModeZero | mgx::kModeRestrict);
            double bytes = 40.0 * k * L.M();
            int kind = MGX_K_GS;
            if (pr) {
                bytes += 32.0 * L.M() + 8.0 * c->lv[l + 1].M();
                kind = MGX_K_PSMOOTH;
            }
            if (rs) bytes += 40.0 * L.M() + 24.0 * c->lv[l + 1].M();
            if (nm) bytes += 48.0 * L.M();
            // compulsory: u (unless zero), rhs, v1, v2 read, u written, the
            // coarse u read (prolong) / coarse rhs written (restrict)
            // (v1 / v2 rows >= vz come from the zero row, not HBM)
            // (generated velocity: the 3-sweep pre / post marches, launch_smooth)
            const bool vgu = mgx::smooth_generates_velocity(A, k, mode);
            // (a packed pre-smoothed u: half a level array per packed side)
            const double cbytes = 8.0 * (((mode & mgx::kModeZero) ? 2.0 : 3.0) * L.M() +
                                         (vgu ? 0.0 : 2.0 * L.Mv()) +
                                         ((pr ? 1 : 0) + (rs ? 1 : 0)) * c->lv[l + 1].M() -
                                         0.5 * L.M() * ((A.pin ? 1 : 0) + (A.pout ? 1 : 0)));
            int blocks = 0;
            CHK(check_coarse_rhs(A, mode));
            const size_t before = c->pending.size();
            CHK(launch(c, kind, l, bytes, cbytes,
                       [&] { blocks = mgx::launch_smooth(A, k, mode, c->stream); }));
            if (blocks < 0) unlaunch(c, before);
            if (blocks == -4 && cfuse) {
                // the pass would march: the coarsest solve on its own, then the pass
                // (nothing was launched)
                A.cf = mgx::CoarseFuse{};
                CHK(flush_coarse(c));
                A.uc = c->lv[l + 1].U();
                CHK(launch(c, kind, l, bytes, cbytes,
                           [&] { blocks = mgx::launch_smooth(A, k, mode, c->stream); }));
            } else if (cfuse) {
                took_coarse(c, l);
            }
            if (blocks < 0) return fail(MGX_E_ARG, "launch_smooth: unsupported sweeps/mode");
            if (l >= 1) L.packed[L.cur] = false;   // (a packed input: consumed)
            L.cur = L.nxt();
            L.packed[L.cur] = A.pout;   // (else whole rows written)
            L.zero = false;
            if (rs) c->lv[l + 1].zero = true;
            if (nm && fused_norm) *fused_norm = true;
            done += k;
        }
        if (prolong && L.zero) CHK(op_prolong_add(c, l));   // unreachable in practice
        return MGX_OK;
    }
    if (prolong) CHK(op_prolong_add(c, l));
    for (int k = 0; k < sweeps; ++k) {
        if (c->opt.smoother == 2) {
            const bool z = L.zero;
            CHK(launch(c, MGX_K_GS, l, 40.0 * L.M(), [&] {
                mgx::launch_gs_sweep(L.u[L.cur], L.u[L.nxt()], L.rhs, L.v1, L.v2, L.n, L.pitch,
                                     L.coef, z, c->stream);
            }));
            L.cur = L.nxt();
            L.zero = false;
        } else {
            CHK(materialize(c, l));
            CHK(launch(c, MGX_K_GS, l, 40.0 * L.M(), [&] {
                mgx::launch_gs_colour(L.U(), L.rhs, L.v1, L.v2, L.n, L.pitch, L.coef, 0,
                                      c->stream);
                mgx::launch_gs_colour(L.U(), L.rhs, L.v1, L.v2, L.n, L.pitch, L.coef, 1,
                                      c->stream);
            }));
        }
    }
    if (restrict_) CHK(op_restrict(c, l));
    return MGX_OK;
}

int op_gs(mgx_ctx *c, int l, int sweeps) {
    return op_smooth(c, l, sweeps, false, false, false, nullptr);
}

// residual + compute_norm on level l, norm read back to the host (the one
// host sync per cycle, gs.cpp:86 / multigrid.cpp:105,113).
int read_norm(mgx_ctx *c, double *norm) {
    HIPCHK(hipMemcpyAsync(c->hscal, c->dscal, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *norm = c->hscal[0];
    return MGX_OK;
}

int op_residual_norm(mgx_ctx *c, int l, double *norm, double bytes_per_pt) {
    CHK(materialize(c, l));
    Level &L = c->lv[l];
    CHK(launch(c, MGX_K_RESNORM, l, bytes_per_pt * L.M(), 32.0 * L.M(), [&] {
        mgx::launch_residual_norm(L.U(), L.rhs, L.v1, L.v2, L.n, L.pitch, L.coef, c->partials,
                                  c->dscal, c->stream);
    }));
    return read_norm(c, norm);
}

// residual -> restriction into rhs[l+1]; u[l+1] = 0 (multigrid.cpp:73-77).
int op_restrict(mgx_ctx *c, int l) {
    CHK(materialize(c, l));
    Level &F = c->lv[l], &C = c->lv[l + 1];
    CHK(launch(c, MGX_K_RESTRICT, l, 40.0 * F.M() + 24.0 * C.M(), 32.0 * F.M() + 8.0 * C.M(), [&] {
        mgx::launch_residual_restrict(F.U(), F.rhs, F.v1, F.v2, F.n, F.pitch, F.coef, C.rhs,
                                      C.pitch, c->stream);
    }));
    C.zero = true;
    return MGX_OK;
}

// u[l] += prolongation(u[l+1]) (multigrid.cpp:81-83).
int op_prolong_add(mgx_ctx *c, int l) {
    CHK(flush_coarse(c));   // a deferred coarsest solve must run before it is prolonged
    CHK(materialize(c, l));
    CHK(materialize(c, l + 1));
    Level &F = c->lv[l], &C = c->lv[l + 1];
    CHK(launch(c, MGX_K_PROLONG, l, 32.0 * F.M() + 8.0 * C.M(), 16.0 * F.M() + 8.0 * C.M(), [&] {
        mgx::launch_prolong_add(F.U(), F.pitch, C.U(), C.pitch, C.n, c->stream);
    }));
    return MGX_OK;
}

// A W-cycle's post-smoothing of visit sh and pre-smoothing of visit sh+1 on
// level l as one tile pass (launch_smooth_wpair): prolongation + add,
// 2 nsmooth sweeps, residual restricted into rhs[l+1], u[l+1] = 0 -- bitwise
// the two passes.  *done = false (nothing launched) where it does not apply.
long g_wpair = 1;   // tuning key "wpair"
int op_wpair(mgx_ctx *c, int l, bool *done) {
    *done = false;
    Level &L = c->lv[l], &Cl = c->lv[l + 1];
    const int k = c->opt.nsmooth;
    if (!g_wpair || c->opt.smoother != 0 || k < 1 || k > 3 || c->opt.fuse < k || L.zero)
        return MGX_OK;
    if (L.packed[L.cur]) return MGX_OK;   // (a march level's packed u: the two passes)
    // The coarsest solve pending, fused: its workgroups read Cl.rhs at their
    // start while the pass's restriction stores the next visit's rhs, so that
    // goes to the level's second rhs buffer (swapped in after the launch);
    // without one the solve runs on its own first.
    if (c->cf_level == l + 1 && !Cl.rhs_alt) CHK(flush_coarse(c));
    const bool cfuse = c->cf_level == l + 1;
    if (Cl.zero && !cfuse) return MGX_OK;
    mgx::SmoothArgs A{};
    A.uin = L.u[L.cur];
    A.uout = L.u[L.nxt()];
    A.rhs = L.rhs;
    A.v1 = L.v1;
    A.v2 = L.v2;
    A.n = L.n;
    A.pitch = L.pitch;
    A.c = L.coef;
    A.uc = Cl.U();
    A.rhsc = cfuse ? Cl.rhs_alt : Cl.rhs;
    A.pitchc = Cl.pitch;
    A.partials = c->partials;
    A.norm_out = c->dscal;
    if (cfuse) take_coarse(c, l, A);
    CHK(check_coarse_rhs(A, mgx::kModeProlong | mgx::kModeRestrict));
    // post (prolong + add, k sweeps) + pre (k sweeps, restrict)
    const double bytes = (32.0 + 40.0 * k) * L.M() + 8.0 * Cl.M() + (40.0 * k + 40.0) * L.M() +
                         24.0 * Cl.M();
    const double cbytes = 8.0 * (3.0 * L.M() + 2.0 * L.Mv() + 2.0 * Cl.M());
    int blocks = 0;
    const size_t before = c->pending.size();
    CHK(launch(c, MGX_K_PSMOOTH, l, bytes, cbytes,
               [&] { blocks = mgx::launch_smooth_wpair(A, k, c->stream); }));
    if (blocks < 0) unlaunch(c, before);   // nothing launched
    if (blocks == -4) return flush_coarse(c);   // the two passes
    if (blocks < 0) return MGX_OK;   // a march level: the two passes as usual
    if (cfuse) {
        took_coarse(c, l);
        std::swap(Cl.rhs, Cl.rhs_alt);   // the restricted rhs is the current one
    }
    L.cur = L.nxt();
    Cl.zero = true;
    *done = true;
    return MGX_OK;
}

// Coarsest level: GS until |r| <= coarse_tol or coarse_maxit (multigrid.cpp:55-65),
// `reps` times in a row (a W-cycle's `shape` visits, multigrid.cpp:52): one
// launch for all of them when the level fits one workgroup.
int op_coarse(mgx_ctx *c, int l, int reps) {
    Level &L = c->lv[l];
    if (L.n <= mgx::kCoarseOneWgMaxN) {
        const bool z = L.zero;
        CHK(launch(c, MGX_K_COARSE, l, 88.0 * L.M() * reps, 40.0 * L.M(), [&] {
            mgx::launch_coarse_solve(L.U(), L.rhs, L.v1, L.v2, L.n, L.pitch, L.coef,
                                     c->opt.coarse_tol, c->opt.coarse_maxit, z, c->dscal + 2,
                                     c->stream, reps);
        }));
        L.zero = false;
        return MGX_OK;
    }
    for (int r = 0; r < reps; ++r) {
        int it = 0;
        double res = 1.0;
        while (it < c->opt.coarse_maxit && res > c->opt.coarse_tol) {
            bool fused = false;
            CHK(op_smooth(c, l, 1, false, false, true, &fused));
            if (fused)
                CHK(read_norm(c, &res));
            else
                CHK(op_residual_norm(c, l, &res, 48.0));
            ++it;
        }
        c->hscal[4] += it;
    }
    return MGX_OK;
}

long g_step_fuse = 1;   // tuning key "step_fuse"

// Can level 0 run the cross-cycle pass (post of cycle k + pre of cycle k+1)?
static bool cross_ok(mgx_ctx *c) {
    const Level &L = c->lv[0];
    return cross_cycle_on() && !c->dist && c->L > 1 && L.u[2] && c->opt.smoother == 0 &&
           c->opt.shape >= 1 && (c->opt.nsmooth == 2 || c->opt.nsmooth == 3) &&
           c->opt.fuse >= c->opt.nsmooth;
}

// The speculative next-cycle state is only valid while nothing but V-cycles
// touches the levels; every other mutating entry point drops it.
// (a packed u_pre is reachable through spec and xin only: it goes with them)
void drop_spec(mgx_ctx *c) {
    if (!c->lv.empty()) {
        Level &L = c->lv[0];
        L.spec = -1;
        if (L.xin >= 0 && L.packed[L.xin]) L.xin = -1;
        if (!L.packed[L.cur]) L.packed[0] = L.packed[1] = L.packed[2] = false;
    }
    c->step_spec = false;
}

// tuning key "xpack": 0 whole rows, 1 packed, 2 (default) packed in fp_mode
// fma inside mgx_run_cycles only -- measured: level 0 -4.8 % there, +5 % in
// the bitwise mode, whose rebuilt colour costs a division per point; and
// mg_outer's last cycle reads whole rows, so there a packed u_pre costs an
// expansion pass per call, more than a few cycles' gain
long g_xpack = 2;

static mgx::XArgs cross_args(mgx_ctx *c) {
    Level &L = c->lv[0], &Cl = c->lv[1];
    mgx::XArgs A;
    A.rhs = L.rhs;
    A.v1 = L.v1;
    A.v2 = L.v2;
    A.uc = Cl.U();
    A.pitchc = Cl.pitch;
    A.rhsc = Cl.rhs;
    A.partials = c->partials;
    A.norm_out = c->dscal;
    A.n = L.n;
    A.pitch = L.pitch;
    A.c = L.coef;
    A.sa1 = L.sa1;
    A.sb1 = L.sb1;
    A.sa2 = L.sa2;
    A.sb2 = L.sb2;
    return A;
}

// Level 0's current buffer in full form, for the passes that read whole rows:
// a packed u_pre is expanded into the ping-pong partner (free wherever this
// is called: the cycle's other two buffers hold a dead u_post and a dead or
// dropped u_pre), which becomes the current buffer.
int op_expand(mgx_ctx *c) {
    Level &L = c->lv[0];
    if (!L.packed[L.cur]) return MGX_OK;
    const int src = L.cur, dst = L.nxt();
    const mgx::XArgs A = cross_args(c);
    // the packed rows, rhs (+ v1, v2) read; the full rows written
    const double cbytes = 8.0 * (2.5 * L.M() + (L.sa1 ? 0.0 : 2.0 * L.M()));
    // (profiled as what it is: half a sweep, 40 B per point a sweep)
    CHK(launch(c, MGX_K_GS, 0, 20.0 * L.M(), cbytes,
               [&] { mgx::launch_xexpand(A, L.u[src], L.u[dst], c->stream); }));
    L.packed[src] = L.packed[dst] = false;
    if (L.xin == src) L.xin = dst;
    L.cur = dst;
    return MGX_OK;
}

// k_xsmooth on level 0: u_post (cycle k, returned by mg_outer if it stops
// here) into one free buffer, u_pre (cycle k+1's pre-smoothing) into the
// other, the residual of u_post -> c->dscal[0], the restriction of u_pre's
// residual -> rhs[1] (u[1] flagged zero for cycle k+1).
static int op_cross(mgx_ctx *c, bool store_post, bool rs = false) {
    Level &L = c->lv[0], &Cl = c->lv[1];
    CHK(materialize(c, 1));
    if (rs && !L.rhs_alt) return fail(MGX_E_INTERNAL, "step-mode cross pass without rhs_alt");
    // u_pre goes out packed (tuning key "xpack") wherever the pass has that
    // form; step mode and the tile form read and write whole rows
    const bool pk_ok = !rs && mgx::xpack_supported(L.n, L.coef.dgs);
    const bool pout = pk_ok && (g_xpack == 1 || (g_xpack == 2 && L.coef.fm && c->fixed_cycles));
    if (!pout) CHK(op_expand(c));   // (a packed input comes with a packed output only)
    const bool pin = L.packed[L.cur];
    int P = -1, Q = -1;
    for (int i = 0; i < 3; ++i)
        if (i != L.cur) (P < 0 ? P : Q) = i;
    mgx::XArgs A = cross_args(c);
    A.uin = L.U();
    A.upost = L.u[P];
    A.upre = L.u[Q];
    A.store_post = store_post;
    A.pin = pin;
    A.pout = pout;
    if (rs) {
        A.rhs_next = L.rhs_alt;
        A.norm2_out = c->dscal + 6;
    }
    const int k = c->opt.nsmooth;
    // algorithmic bytes: prolong+add, k sweeps, residual+norm (post of cycle
    // k) + k sweeps, residual+restriction (pre of cycle k+1), SURVEY 8d
    const double bytes = (32.0 + 40.0 * k + 48.0) * L.M() + 8.0 * Cl.M() +
                         (40.0 * k + 40.0) * L.M() + 24.0 * Cl.M();
    // compulsory: u, rhs, v1, v2 and the coarse u read once; u_pre (+ u_post)
    // and the coarse rhs written once
    // (step mode: + compute_rhs and the initial residual norm of the next
    // step, and its rhs written)
    // (with velocity factors v1 / v2 are not read: two fine arrays fewer)
    const double bytes_rs = rs ? (32.0 + 48.0) * L.M() : 0.0;
    // (a packed u_pre: half a fine array per packed side)
    const double cbytes = 8.0 * ((store_post ? 6.0 : 5.0) * L.M() - (L.sa1 ? 2.0 * L.M() : 0.0) +
                                 2.0 * Cl.M() + (rs ? L.M() : 0.0) -
                                 0.5 * L.M() * ((pin ? 1 : 0) + (pout ? 1 : 0)));
    int blocks = 0;
    CHK(launch(c, MGX_K_XSMOOTH, 0, bytes + bytes_rs, cbytes,
               [&] { blocks = mgx::launch_xsmooth(A, k, c->stream); }));
    if (blocks < 0) return fail(MGX_E_ARG, "launch_xsmooth: unsupported sweeps / mode");
    L.xin = L.cur;
    L.cur = P;
    L.spec = Q;
    L.packed[P] = false;
    L.packed[Q] = pout;
    L.zero = false;
    Cl.zero = true;
    return MGX_OK;
}

// mg_inner (multigrid.cpp:17-92).  If norm != nullptr (finest level only) the
// residual norm after the cycle (multigrid.cpp:112-113) is produced too, fused
// into the last post-smoothing pass when possible.
//
// Finest level with a norm (mg_outer's cycles): the post-smoothing of this
// cycle and the pre-smoothing of the NEXT one are one k_xsmooth pass, so a
// cycle is [pre (first cycle only) | coarse levels | cross pass]; a cycle that
// follows one starts from the speculative state the cross pass left.
// W-cycles (shape 2, multigrid.cpp:52): visit sh's post-smoothing of level 0
// and visit sh+1's pre-smoothing + restriction are adjacent too, so they are
// one cross pass as well (its u_post and norm unused): [pre | coarse | cross |
// coarse | cross] per W-cycle instead of four level-0 passes.
// tuning key "graph_level": > 0 = op_vcycle(c, graph_level) -- the whole
// sub-cycle of the small levels below a level: their tile / march passes and
// the coarsest solve -- is captured once per entry state as a hipGraph
// (hipStreamBeginCapture on the context's own stream) and replayed, one
// hipGraphLaunch instead of ~10 (V) or ~1000 (W) kernel launches; 0 (default)
// = launched one by one.  The round-6 kernel trace has no idle time between
// the launches of a cycle (profiles/r6_gaps_*.txt), so this only moves host
// work.  Not with per-launch profiling (prof 1; prof 2 times level 0 only),
// partitioned contexts or a borrowed stream, nor
// where the coarsest solve loops on the host (n > kCoarseOneWgMaxN).
long g_graph_level = 0;
long g_tuning_epoch = 0;   // bumped by every mgx_set_tuning: graphs of older settings are stale
long g_graph_captures = 0, g_graph_replays = 0;   // (read-only keys, for the tests)

// The host state a sub-cycle from level l reads and changes: per level its
// current u buffer, zero flag and rhs buffers, the deferred coarsest solve,
// and the process tuning epoch.  Equal keys = the same launches on the same
// buffers (everything else the passes read is fixed at creation / upload).
static std::vector<long> graph_state(const mgx_ctx *c, int l) {
    std::vector<long> k;
    for (int i = l; i < c->L; ++i) {
        const Level &L = c->lv[i];
        k.push_back(L.cur);
        k.push_back(L.zero ? 1 : 0);
        k.push_back((long)(uintptr_t)L.rhs);
        k.push_back((long)(uintptr_t)L.rhs_alt);
    }
    k.push_back(c->cf_level);
    k.push_back(c->cf_reps);
    k.push_back(g_tuning_epoch);
    return k;
}
static void set_graph_state(mgx_ctx *c, int l, const std::vector<long> &k) {
    size_t j = 0;
    for (int i = l; i < c->L; ++i) {
        Level &L = c->lv[i];
        L.cur = (int)k[j++];
        L.zero = k[j++] != 0;
        L.rhs = (double *)(uintptr_t)k[j++];
        L.rhs_alt = (double *)(uintptr_t)k[j++];
    }
    c->cf_level = (int)k[j++];
    c->cf_reps = (int)k[j++];
}
static bool graphable(const mgx_ctx *c, int l) {
    return g_graph_level > 0 && l == g_graph_level && !c->capturing && !c->dist &&
           c->own_stream && c->prof != 1 && c->opt.smoother == 0 && l >= 1 && l < c->L - 1 &&
           c->lv[c->L - 1].n <= mgx::kCoarseOneWgMaxN;
}
void free_graphs(mgx_ctx *c) {
    for (auto &g : c->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    c->graphs.clear();
}
static int graph_vcycle(mgx_ctx *c, int l) {
    const std::vector<long> key = graph_state(c, l);
    for (auto &g : c->graphs)
        if (g.key == key) {
            HIPCHK(hipGraphLaunch(g.exec, c->stream));
            set_graph_state(c, l, g.end);
            ++g_graph_replays;
            return MGX_OK;
        }
    if (c->graphs.size() >= 8) free_graphs(c);   // (stale entry states: start over)
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    c->capturing = true;
    const int rc = op_vcycle(c, l);
    c->capturing = false;
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(c->stream, &graph);
    if (rc != MGX_OK) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
    }
    if (e != hipSuccess) return fail(MGX_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    mgx_ctx::Graph g;
    g.key = key;
    g.end = graph_state(c, l);
    const hipError_t ei = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) return fail(MGX_E_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
    c->graphs.push_back(g);
    ++g_graph_captures;
    // (the capture only recorded the launches: run them now)
    HIPCHK(hipGraphLaunch(g.exec, c->stream));
    return MGX_OK;
}

int op_vcycle(mgx_ctx *c, int l, double *norm, bool store_post) {
    if (!norm && graphable(c, l)) return graph_vcycle(c, l);
    if (l == 0 && norm && cross_ok(c)) {
        Level &L = c->lv[0];
        if (L.spec >= 0) {   // pre-smoothing + restriction already done
            L.cur = L.spec;
            L.spec = -1;
        } else {
            CHK(op_smooth(c, 0, c->opt.nsmooth, false, /*restrict=*/true, false, nullptr));
        }
        for (int sh = 1; sh < c->opt.shape; ++sh) {
            CHK(op_vcycle(c, 1));
            CHK(op_cross(c, /*store_post=*/false));
            L.cur = L.spec;   // visit sh+1 starts from the pass's u_pre
            L.spec = -1;
        }
        CHK(op_vcycle(c, 1));
        if (c->post_only && c->step_next && mgx::xstep_supported(L.n) && L.coef.dgs > 0) {
            // the last cycle of a time step whose next step follows: the cross
            // pass in step mode (u_post stored; B pre-smooths the next step)
            CHK(op_cross(c, /*store_post=*/true, /*rs=*/true));
            HIPCHK(hipMemcpyAsync(c->hscal, c->dscal, sizeof(double), hipMemcpyDeviceToHost,
                                  c->stream));
            HIPCHK(hipMemcpyAsync(c->hscal + 6, c->dscal + 6, sizeof(double),
                                  hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            *norm = c->hscal[0];
            c->step_res0 = c->hscal[6];
            c->step_spec = true;
            return MGX_OK;
        }
        if (c->post_only) {   // the last cycle: prolongation + post-smoothing + norm only
            bool fused = false;
            CHK(op_expand(c));   // (k_wsmooth reads whole rows)
            CHK(op_smooth(c, 0, c->opt.nsmooth, /*prolong=*/true, false, /*norm=*/true, &fused));
            L.spec = -1;
            return fused ? read_norm(c, norm) : op_residual_norm(c, 0, norm);
        }
        CHK(op_cross(c, store_post));
        return read_norm(c, norm);
    }
    if (l == 0) drop_spec(c);
    bool have_norm = false;
    bool pre_done = false;   // visit sh's pre-smoothing ran fused with sh-1's post
    // (the coarsest level's `shape` solves in a row: one op_coarse)
    for (int sh = 0; sh < (l == c->L - 1 ? 1 : c->opt.shape); ++sh) {
        const bool last = sh == c->opt.shape - 1;
        if (l == c->L - 1) {
            if (coarse_fusable(c, l)) {   // taken by the next prolongation pass
                c->cf_level = l;
                c->cf_reps = c->opt.shape;
            } else {
                CHK(op_coarse(c, l, c->opt.shape));
            }
        } else {
            // (the next reader of u[l] is this visit's post-smoothing below:
            // levels >= 1 may hand it over as one colour, "wpack")
            if (!pre_done)
                CHK(op_smooth(c, l, c->opt.nsmooth, false, /*restrict=*/true, false, nullptr,
                              /*pack_out=*/l >= 1));
            pre_done = false;
            CHK(op_vcycle(c, l + 1));
            // W-cycles: this visit's post- and the next visit's pre-smoothing
            // back to back -- one tile pass where the level runs as tiles
            if (!last) {
                bool fused = false;
                CHK(op_wpair(c, l, &fused));
                if (fused) {
                    pre_done = true;
                    continue;
                }
            }
            CHK(op_smooth(c, l, c->opt.nsmooth, /*prolong=*/true, false, norm && last,
                          &have_norm));
            CHK(flush_coarse(c));   // (taken above; never left pending)
        }
    }
    if (norm) {
        if (have_norm)
            CHK(read_norm(c, norm));
        else
            CHK(op_residual_norm(c, l, norm));
    }
    return MGX_OK;
}

// tuning key "source_sv": 1 (default) = the source pass of a context that keeps
// finest-level velocity factors forms v1, v2 from them; 0 = always reads the
// 2-D arrays (bitwise the same)
long g_source_sv = 1;

// The source pass (source.hip) on a single-GPU context's finest level; the
// factor variant is chosen per launch (a velocity replacement can add or
// remove the factors).  norm: also the residual norm against the new rhs into
// c->dscal[0].  *cbytes: the arrays the launch reads or writes, once.
static mgxsrc::SrcArgs source_args(mgx_ctx *c, bool norm, double *cbytes) {
    Level &L = c->lv[0];
    mgxsrc::SrcArgs A;
    A.rhs = L.rhs;
    A.u = L.U();
    A.v1 = L.v1;
    A.v2 = L.v2;
    A.f = c->src;
    A.terms = c->src_terms;   // > 0: the separable form, no f stream
    A.fa = c->src_a;
    A.fb = c->src_b;
    A.cf = c->dt * c->src_scale;
    A.n = L.n;
    A.pitch = L.pitch;
    A.c = L.coef_rhs;   // (== coef while kA == kB: the norm instance needs that)
    const bool sv = g_source_sv != 0 && L.sa1 && L.sb1 && L.sa2 && L.sb2;
    if (sv) {
        A.sa1 = L.sa1;
        A.sb1 = L.sb1;
        A.sa2 = L.sa2;
        A.sb2 = L.sb2;
    }
    if (norm) {
        A.partials = c->partials;
        A.norm_out = c->dscal;
    }
    // u, rhs (+ f unless separable) (+ v1, v2)
    *cbytes = ((sv ? 16.0 : 32.0) + (A.terms ? 0.0 : 8.0)) * L.M();
    return A;
}

int op_rhs(mgx_ctx *c) {
    drop_spec(c);
    CHK(materialize(c, 0));
    Level &L = c->lv[0];
    if (c->has_source()) {   // compute_rhs 32 B per point + the f stream of a field
        double cb = 0;
        const mgxsrc::SrcArgs A = source_args(c, false, &cb);
        return launch(c, MGX_K_RHS, 0, (A.terms ? 32.0 : 40.0) * L.M(), cb,
                      [&] { mgxsrc::launch_rhs_source(A, c->stream); });
    }
    return launch(c, MGX_K_RHS, 0, 32.0 * L.M(), [&] {
        mgx::launch_rhs(L.rhs, L.U(), L.v1, L.v2, L.n, L.pitch, L.coef_rhs, c->stream);
    });
}

// compute_rhs (gs.cpp:24) + mg_outer's initial residual norm (multigrid.cpp:104)
// in one pass over u, v1, v2 (a time step's first two reads of the fields)
static int op_rhs_norm(mgx_ctx *c, double *res0) {
    drop_spec(c);
    CHK(materialize(c, 0));
    Level &L = c->lv[0];
    if (c->has_source()) {
        double cb = 0;
        const mgxsrc::SrcArgs A = source_args(c, true, &cb);
        CHK(launch(c, MGX_K_RHS, 0, (A.terms ? 32.0 : 40.0) * L.M() + 48.0 * L.M(), cb,
                   [&] { mgxsrc::launch_rhs_source(A, c->stream); }));
        return read_norm(c, res0);
    }
    CHK(launch(c, MGX_K_RHS, 0, 32.0 * L.M() + 48.0 * L.M(), 32.0 * L.M(), [&] {
        mgx::launch_rhs_norm(L.rhs, L.U(), L.v1, L.v2, L.n, L.pitch, L.coef, c->partials,
                             c->dscal, c->stream);
    }));
    return read_norm(c, res0);
}

// The same for a step whose two sides differ (mgx_ctx::two_op, theta != 1/2):
// rhs = B(kB) u (+ the source term) and the norm of rhs - A(kA) u in one pass
// (csrc/tstep.hip) -- the fused kernels above form both from one Coef.
static int op_rhs_norm2(mgx_ctx *c, double *res0) {
    drop_spec(c);
    CHK(materialize(c, 0));
    Level &L = c->lv[0];
    double cb = 0;
    const mgxsrc::SrcArgs A = source_args(c, true, &cb);   // (f and terms unset: no source)
    const bool field = A.f && !A.terms;
    // u, rhs (+ f of a field source) (+ v1, v2 without factors)
    cb = ((A.sa1 ? 16.0 : 32.0) + (field ? 8.0 : 0.0)) * L.M();
    CHK(launch(c, MGX_K_RHS, 0, (field ? 40.0 : 32.0) * L.M() + 48.0 * L.M(), cb,
               [&] { mgxts::launch_rhs_norm2(A, L.coef, c->stream); }));
    return read_norm(c, res0);
}

// The first pass of a BDF2 step (csrc/bdf.hip): rhs = b0 u - b1 h (+ cf f), u
// stored over h on the whole array, and the norm of rhs - A u with the level's
// coef (the caller has built it with kA) in one march.
int op_rhs_norm_bdf(mgx_ctx *c, double b0, double b1, double cf, double *res0) {
    drop_spec(c);
    CHK(materialize(c, 0));
    CHK(op_expand(c));   // (as mgx_download: h becomes what it would return)
    Level &L = c->lv[0];
    double cb = 0;
    mgxsrc::SrcArgs A = source_args(c, true, &cb);   // (f and terms unset: no source)
    A.c = L.coef;
    A.cf = cf;
    const bool field = A.f && !A.terms;
    // u and h in, h and rhs out (+ f of a field source) (+ v1, v2 without factors)
    cb = ((A.sa1 ? 32.0 : 48.0) + (field ? 8.0 : 0.0)) * L.M();
    // depth 2: the caller has exchanged the two arrays (hist_swap), u^(n-1) is
    // read from hist2 and u^n stored into hist -- the same bytes
    const double *hin = c->hist2 ? c->hist2 : c->hist;
    CHK(launch(c, MGX_K_RHS, 0, (field ? 96.0 : 88.0) * L.M(), cb,
               [&] { mgxbdf::launch_rhs_norm_bdf(A, hin, c->hist, b0, b1, c->stream); }));
    return read_norm(c, res0);
}

// The same pass with a predicted start (csrc/predict.hip): the guess goes to the
// free buffer of level 0 (free wherever op_rhs_norm_pre's is), nothing is stored
// into the history, and two norms come back in one read.
int op_predict_bdf(mgx_ctx *c, double b0, double b1, double cf, int e, const double w[3],
                   double *res0, double *resp) {
    drop_spec(c);
    CHK(materialize(c, 0));
    CHK(op_expand(c));   // (as mgx_download: h becomes what it would return)
    Level &L = c->lv[0];
    double cb = 0;
    mgxsrc::SrcArgs A = source_args(c, true, &cb);   // (f and terms unset: no source)
    A.c = L.coef;
    A.cf = cf;
    const bool field = A.f && !A.terms;
    // u, h (, h2) in, g and rhs out (+ f of a field source) (+ v1, v2 without factors)
    cb = (8.0 * (3 + e) + (A.sa1 ? 0.0 : 16.0) + (field ? 8.0 : 0.0)) * L.M();
    // the BDF pass, the second residual, the guess (e + 1 reads, one write)
    const double bytes = ((field ? 96.0 : 88.0) + 48.0 + 8.0 * (e + 2)) * L.M();
    double *gout = L.u[L.nxt()];
    CHK(launch(c, MGX_K_RHS, 0, bytes, cb, [&] {
        mgxpred::launch_predict_bdf(A, c->hist, e == 2 ? c->hist2 : nullptr, e, w, gout, b0, b1,
                                    c->stream);
    }));
    L.packed[L.nxt()] = false;
    HIPCHK(hipMemcpyAsync(c->hscal, c->dscal, 2 * sizeof(double), hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *res0 = c->hscal[0];
    *resp = c->hscal[1];
    return MGX_OK;
}

// mgx_set_history on one context's own state
int hist_alloc_ctx(mgx_ctx *c, const char *who) {
    if (c->hist) return MGX_OK;
    const Level &L = c->lv[0];
    const size_t bytes = sizeof(double) * (size_t)(L.n + 1) * (size_t)L.pitch;
    const hipError_t e = hipMalloc(&c->hist, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        c->hist = nullptr;
        return fail(MGX_E_HIP, std::string(who) + ": no room for the history (one finest-level "
                                                  "array): " + hipGetErrorString(e));
    }
    return MGX_OK;
}
void hist_free_ctx(mgx_ctx *c) {
    if (!c->hist) return;
    (void)hipStreamSynchronize(c->stream);   // a pass may still read it
    (void)hipFree(c->hist);
    c->hist = nullptr;
    (void)hipFree(c->hist2);
    c->hist2 = nullptr;
}
int hist2_alloc_ctx(mgx_ctx *c, bool zero_hist, const char *who) {
    const Level &L = c->lv[0];
    const size_t bytes = sizeof(double) * (size_t)(L.n + 1) * (size_t)L.pitch;
    if (!c->hist2) {
        hipError_t e = hipMalloc(&c->hist2, bytes);
        if (e == hipSuccess && (e = hipMemsetAsync(c->hist2, 0, bytes, c->stream)) != hipSuccess)
            (void)hipFree(c->hist2);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            c->hist2 = nullptr;
            return fail(MGX_E_HIP, std::string(who) + ": no room for the second history array "
                                                      "(one finest-level array): " +
                                       hipGetErrorString(e));
        }
    }
    if (zero_hist) HIPCHK(hipMemsetAsync(c->hist, 0, bytes, c->stream));
    return MGX_OK;
}
void hist2_free_ctx(mgx_ctx *c) {
    if (!c->hist2) return;
    (void)hipStreamSynchronize(c->stream);   // a pass may still read it
    (void)hipFree(c->hist2);
    c->hist2 = nullptr;
}
void hist_swap(mgx_ctx *c) {
    if (c->dist)
        dist_hist_swap(c);
    else
        std::swap(c->hist, c->hist2);
}
int hist_snapshot_ctx(mgx_ctx *c) {
    CHK(materialize(c, 0));
    CHK(op_expand(c));   // as mgx_download
    const Level &L = c->lv[0];
    const size_t bytes = sizeof(double) * (size_t)(L.n + 1) * (size_t)L.pitch;
    HIPCHK(hipMemcpyAsync(c->hist, L.U(), bytes, hipMemcpyDeviceToDevice, c->stream));
    return MGX_OK;
}
int hist_restore_ctx(mgx_ctx *c) {
    CHK(boundary_prepare_ctx(c));
    const Level &L = c->lv[0];
    const size_t bytes = sizeof(double) * (size_t)(L.n + 1) * (size_t)L.pitch;
    HIPCHK(hipMemcpyAsync(L.U(), c->hist, bytes, hipMemcpyDeviceToDevice, c->stream));
    return MGX_OK;
}

// A time step's compute_rhs, mg_outer's initial norm AND the first cycle's
// pre-smoothing + restriction in ONE pass over u, v1, v2 (k_wsmooth mode
// kModeRhsNorm): u_pre goes to the free buffer and is left as the
// speculative state the first cycle starts from (Level::spec, as after a
// cross pass).  Only where the cross-cycle schedule runs (so the first cycle
// takes that state) and level 0 is a row march.  -> false: not applicable.
static bool step_fusable(mgx_ctx *c) {
    return cross_ok(c) && c->lv[0].n > mgx::get_tile_max_n() && g_step_fuse != 0;
}
static int op_rhs_norm_pre(mgx_ctx *c, double *res0) {
    drop_spec(c);
    CHK(materialize(c, 0));
    CHK(materialize(c, 1));
    Level &L = c->lv[0], &Cl = c->lv[1];
    const int k = c->opt.nsmooth;
    const int out = L.nxt();
    mgx::SmoothArgs A{};
    A.uin = L.u[L.cur];
    A.uout = L.u[out];
    A.rhs = L.rhs;
    A.rhs_out = L.rhs;
    A.v1 = L.v1;
    A.v2 = L.v2;
    A.n = L.n;
    A.pitch = L.pitch;
    A.c = L.coef;
    A.uc = Cl.U();
    A.rhsc = Cl.rhs;
    A.pitchc = Cl.pitch;
    A.partials = c->partials;
    A.norm_out = c->dscal;
    // algorithmic: compute_rhs 32, residual+norm 48, k sweeps 40 each,
    // residual+restriction 40 + 24 per coarse point; compulsory: u, v1, v2
    // read, rhs and u_pre written, the coarse rhs written
    const double bytes = (32.0 + 48.0 + 40.0 * k + 40.0) * L.M() + 24.0 * Cl.M();
    const double cbytes = 8.0 * (5.0 * L.M() + Cl.M());
    int blocks = 0;
    CHK(launch(c, MGX_K_RHS, 0, bytes, cbytes, [&] {
        blocks = mgx::launch_smooth(A, k, mgx::kModeRestrict | mgx::kModeRhsNorm, c->stream);
    }));
    if (blocks < 0) return fail(MGX_E_ARG, "launch_smooth: rhs+norm+pre-smoothing unsupported");
    L.spec = out;   // the first cycle's pre-smoothed u (op_vcycle takes it)
    L.packed[out] = false;
    L.zero = false;
    Cl.zero = true;
    return read_norm(c, res0);
}

// mg_outer (multigrid.cpp:97-120).
// one V-cycle + the residual norm after it, single GPU or partitioned
// store_post = false: the caller runs another cycle right away, so this
// cycle's solution is never observed (only its norm); skip writing it
int cycle_norm(mgx_ctx *c, double *res, bool store_post = true) {
    if (c->dist) return dist_vcycle(c, res, store_post);
    return op_vcycle(c, 0, res, store_post);
}
int norm0(mgx_ctx *c, double *res) {
    if (c->dist) return dist_residual_norm(c, res);
    return op_residual_norm(c, 0, res);
}

// have_res0: the caller computed the initial norm (fused with compute_rhs)
// The cycle that converged did not store its u_post (predicted to go on):
// recompute it from the cycle's input and the level-1 correction, both still
// intact -- the post-smoothing pass alone, bitwise the cross pass's u_post
// (the same prolongation and sweeps: tests/test_gpu_cross.py).
static int op_redo_post(mgx_ctx *c) {
    Level &L = c->lv[0];
    if (L.xin < 0) return fail(MGX_E_INTERNAL, "redo post-smoothing: no cross pass input");
    L.cur = L.xin;
    L.spec = -1;
    L.zero = false;
    CHK(op_expand(c));   // (the pass's input was a packed u_pre: k_wsmooth reads whole rows)
    c->lv[1].zero = false;   // u[1] still holds the correction the pass prolonged
    return op_smooth(c, 0, c->opt.nsmooth, /*prolong=*/true, false, false, nullptr);
}

// op_vcycle / dist_vcycle with a norm would run the cross-cycle pass
static bool post_predictable(mgx_ctx *c) {
    if (!c->dist) return cross_ok(c);
    if (dist_la(c) == 0) return cross_ok(dist_sub(c, 0));   // everything replicated
    return dist_post_predictable(c);
}
static int redo_post(mgx_ctx *c) {
    if (!c->dist) return op_redo_post(c);
    if (dist_la(c) == 0) {
        for (int i = 0; i < dist_nsub(c); ++i) CHK(op_redo_post(dist_sub(c, i)));
        return MGX_OK;
    }
    return dist_redo_post(c);
}

static void set_post_only(mgx_ctx *c, bool v) {
    c->post_only = v;
    if (c->dist)
        for (int i = 0; i < dist_nsub(c); ++i) dist_sub(c, i)->post_only = v;
}

// tuning key "post_only": a cycle whose extrapolated norm is within tol /
// post_only (or the last cycle mg_outer may run) skips the next cycle's
// pre-smoothing: its finest level runs the post-smoothing pass alone, not the
// cross pass (2.7 GB of u_pre + coarse rhs writes and B's sweeps saved); if it
// does not converge after all, the next cycle pre-smooths from its u_post
// (0 = never; -1 = every cycle, the test of that path)
long g_post_only = 10;

// tuning key "post_predict": mg_outer stores a cycle's u_post only when the
// cycle is predicted to converge -- its norm extrapolated with the last
// reduction factor within post_predict x tol -- and recomputes it in the
// rare case a cycle converges unannounced (0 = always store; -1 = never
// store, always recompute: the test of the recompute path)
double g_post_predict = 10.0;

// start_res: the norm of the u the loop starts from where that is not the u of
// res0 (a predicted start, mgx_set_predictor): the criterion keeps res0, the
// loop and the extrapolation of "post_predict" / "post_only" begin at start_res
int op_mg_outer(mgx_ctx *c, double tol, int *cycles, double *res0_out, double *res_out,
                const double *have_res0 = nullptr, const double *start_res = nullptr) {
    double res0 = 0, res = 0;
    if (have_res0)
        res0 = *have_res0;
    else
        CHK(norm0(c, &res0));
    res = start_res ? *start_res : res0;
    int iter = 0;
    // the u_post of a cycle that does not converge is never observed: the
    // cross pass skips storing it (2.15 GB at N=16384) when so predicted
    const bool predict = g_post_predict != 0 && post_predictable(c);
    double prev = res;
    for (; iter < c->opt.max_cycle && res / res0 > tol; ++iter) {
        bool store = true, last = false;
        if (predict) {
            const double pred = res * (res / prev);
            if (iter + 1 < c->opt.max_cycle)   // the last allowed cycle always stores
                store = g_post_predict > 0 && pred <= g_post_predict * tol * res0;
            last = g_post_only < 0 ||
                   (g_post_only > 0 && (iter + 1 == c->opt.max_cycle ||
                                        pred * (double)g_post_only <= tol * res0));
        }
        prev = res;
        set_post_only(c, last);
        const int rc = cycle_norm(c, &res, store);
        set_post_only(c, false);
        CHK(rc);
        if (c->step_spec && res / res0 > tol) {
            // step mode, but the cycle did not converge: its pre-smoothing was
            // the next step's (other rhs); the next cycle pre-smooths from u_post
            c->step_spec = false;
            c->lv[0].spec = -1;
        }
        if (!store && !last && !(res / res0 > tol)) CHK(redo_post(c));
    }
    if (cycles) *cycles = iter;
    if (res0_out) *res0_out = res0;
    if (res_out) *res_out = res;
    if (iter == c->opt.max_cycle) return fail(MGX_E_NOCONV, "mg_outer did not converge");
    return MGX_OK;
}

// Coarse velocity tower (multigrid.cpp:148-160).  Reference mode reproduces
// the reference's index arithmetic on flat (n/2+1)^2 buffers, zero filled
// (SURVEY K2); correct mode injects every level from the one above.
int build_tower(mgx_ctx *c) {
    const long N = c->N;
    for (int f = 0; f < 2; ++f) {
        double *fine = f == 0 ? c->lv[0].v1 : c->lv[0].v2;
        if (c->opt.tower_mode == MGX_TOWER_CORRECT) {
            for (int l = 1; l < c->L; ++l) {
                Level &A = c->lv[l - 1], &B = c->lv[l];
                const double *src = f == 0 ? A.v1 : A.v2;
                double *dst = f == 0 ? B.v1 : B.v2;
                mgx::launch_injection(dst, B.pitch, src, A.pitch, B.n + 1, c->stream);
                CHK(check_launch("injection"));
            }
            continue;
        }
        if (c->L < 2) continue;
        // flat level-0 copy of the fine field in the reference layout
        HIPCHK(hipMemcpy2DAsync(c->stage[0], (N + 1) * sizeof(double), fine,
                                c->lv[0].pitch * sizeof(double), (N + 1) * sizeof(double), N + 1,
                                hipMemcpyDeviceToDevice, c->stream));
        const long ni = (N >> 1) + 1;   // multigrid.cpp:150
        for (int l = 1; l < c->L; ++l) {
            double *prev = c->stage[(l - 1) & 1], *next = c->stage[l & 1];
            HIPCHK(hipMemsetAsync(next, 0, sizeof(double) * ni * ni, c->stream));
            // restriction(vtow[l], vtow[l-1], ni-1): next[I*(ni/2... )] per gs.cpp:283
            const long nr = ni - 1;   // the "n" passed to restriction
            mgx::launch_injection(next, nr / 2 + 1, prev, nr + 1, nr / 2 + 1, c->stream);
            CHK(check_launch("tower injection"));
            Level &B = c->lv[l];
            double *dst = f == 0 ? B.v1 : B.v2;
            // level l reads its buffer with its own width n_l+1 (multigrid.cpp:46-47)
            HIPCHK(hipMemcpy2DAsync(dst, B.pitch * sizeof(double), next,
                                    (B.n + 1) * sizeof(double), (B.n + 1) * sizeof(double),
                                    B.n + 1, hipMemcpyDeviceToDevice, c->stream));
        }
    }
    return MGX_OK;
}

// tuning key "zero_rows": 1 (default) = find_zero_rows at upload; 0 = read
// every velocity row from HBM
long g_zero_rows = 1;

int find_zero_rows(mgx_ctx *c) {
    for (auto &L : c->lv) L.vz = 0x7fffffff;
    if (c->L < 2 || !g_zero_rows) return MGX_OK;
    int *dflags = nullptr;
    const long nmax = c->lv[1].n + 1;
    HIPCHK(hipMalloc(&dflags, sizeof(int) * 2 * nmax));
    std::vector<int> h(2 * nmax);
    int rc = MGX_OK;
    for (int l = 1; l < c->L && rc == MGX_OK; ++l) {
        Level &L = c->lv[l];
        mgx::launch_row_nonzero(L.v1, L.pitch, L.n, dflags, c->stream);
        mgx::launch_row_nonzero(L.v2, L.pitch, L.n, dflags + nmax, c->stream);
        if (check_launch("row_nonzero") != MGX_OK ||
            hipMemcpyAsync(h.data(), dflags, sizeof(int) * 2 * nmax, hipMemcpyDeviceToHost,
                           c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) {
            rc = fail(MGX_E_HIP, "find_zero_rows");
            break;
        }
        long last = -1;
        for (long i = 0; i <= L.n; ++i)
            if (h[i] || h[nmax + i]) last = i;
        L.vz = (int)(last + 1);
    }
    (void)hipFree(dflags);
    return rc;
}

// The coarse levels that generate their velocity (Level::vgen): levels 1-2 of
// the reference tower (the injection quirk's closed form) or every level of
// the correct tower (strided: the finest factors at rows / columns 2^l i,
// 2^l j), below the coarsest (whose solve reads the arrays), when the finest
// factors exist and every entry of the level equals the generator's bits
// (k_vgen_check).  a1, a2: the finest row factors.
int find_vgen(mgx_ctx *c, const std::vector<double> &a1, const std::vector<double> &a2) {
    for (auto &L : c->lv) L.vgen = false;
    (void)hipFree(c->vga);
    c->vga = nullptr;
    const Level &F = c->lv[0];
    const bool strided = c->opt.tower_mode == MGX_TOWER_CORRECT;
    // (the reference closed form's integer products fit in int up to N = 2^15)
    if (!F.sa1 || c->L < 3 || (c->N & 3) || (!strided && c->N > 32768) ||
        (long)a1.size() != c->N + 1 || (long)a2.size() != c->N + 1)
        return MGX_OK;
    std::vector<double2> h((size_t)c->N + 2, make_double2(0.0, 0.0));
    for (long I = 0; I <= c->N; ++I) h[(size_t)I] = make_double2(a1[(size_t)I], a2[(size_t)I]);
    HIPCHK(hipMalloc(&c->vga, sizeof(double2) * h.size()));
    const int top = strided ? c->L - 2 : std::min(c->L - 2, 2);
    std::vector<int> ok(c->L, 0), one(c->L, 1);
    int *dok = nullptr;
    HIPCHK(hipMalloc(&dok, sizeof(int) * c->L));
    int rc = MGX_OK;
    if (hipMemcpyAsync(c->vga, h.data(), sizeof(double2) * h.size(), hipMemcpyHostToDevice,
                       c->stream) != hipSuccess ||
        hipMemcpyAsync(dok, one.data(), sizeof(int) * c->L, hipMemcpyHostToDevice, c->stream) !=
            hipSuccess)
        rc = fail(MGX_E_HIP, "find_vgen");
    for (int l = 1; l <= top && rc == MGX_OK; ++l) {
        const Level &L = c->lv[l];
        if ((L.n << l) != c->N || (L.n & 1)) continue;
        mgx::launch_vgen_check(L.v1, L.v2, L.n, L.pitch, level_vgen(c, l), dok + l, c->stream);
        rc = check_launch("vgen_check");
    }
    if (rc == MGX_OK &&
        (hipMemcpyAsync(ok.data(), dok, sizeof(int) * c->L, hipMemcpyDeviceToHost, c->stream) !=
             hipSuccess ||
         hipStreamSynchronize(c->stream) != hipSuccess))
        rc = fail(MGX_E_HIP, "find_vgen");
    (void)hipFree(dok);
    bool any = false;
    for (int l = 1; l <= top && rc == MGX_OK; ++l) {
        Level &L = c->lv[l];
        L.vgen = (L.n << l) == c->N && !(L.n & 1) && ok[l] == 1;
        any = any || L.vgen;
    }
    if (!any) {
        (void)hipFree(c->vga);
        c->vga = nullptr;
    }
    return rc;
}

void free_ctx(mgx_ctx *c) {
    if (!c) return;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->dist) dist_free(c);
    for (auto &L : c->lv) {
        (void)hipFree(L.u[0]);
        (void)hipFree(L.u[1]);
        (void)hipFree(L.u[2]);
        (void)hipFree(L.rhs);
        (void)hipFree(L.rhs_alt);
        (void)hipFree(L.v1);
        (void)hipFree(L.v2);
        free_level_factors(L);
    }
    (void)hipFree(c->partials);
    (void)hipFree(c->dscal);
    (void)hipFree(c->stage[0]);
    (void)hipFree(c->stage[1]);
    (void)hipFree(c->zrow);
    (void)hipFree(c->vga);
    (void)hipFree(c->src);
    (void)hipFree(c->src_a);
    (void)hipFree(c->src_b);
    (void)hipFree(c->diag);
    (void)hipFree(c->dense_buf);
    (void)hipFree(c->bc_buf);
    (void)hipFree(c->hist);
    (void)hipFree(c->hist2);
    c->bc_timer.destroy();
    if (c->hscal) (void)hipHostFree(c->hscal);
    for (auto &r : c->pending) {
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    for (auto e : c->pool) (void)hipEventDestroy(e);
    free_graphs(c);
    if (c->stream && c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

bool is_pow2(long n) { return n >= 2 && (n & (n - 1)) == 0; }

// raw-op scratch (norm partials + result), shared by the gs.h-mirror entry points
std::mutex g_raw_mu;
double *g_raw_scratch = nullptr;
int g_raw_dev = -1;

int raw_scratch(double **p) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (!g_raw_scratch || g_raw_dev != dev) {
        HIPCHK(hipMalloc(&g_raw_scratch, sizeof(double) * (mgx::norm_partials_size() + 8)));
        g_raw_dev = dev;
    }
    *p = g_raw_scratch;
    return MGX_OK;
}

}  // namespace mgxi

using namespace mgxi;

// =================================================================== C ABI
extern "C" {

const char *mgx_last_error(void) { return g_err.c_str(); }
int mgx_version(void) { return 100; }

void mgx_default_options(mgx_options *o) {
    o->nsmooth = 3;          // multigrid.cpp:41
    o->shape = 1;            // multigrid.cpp:241
    o->tower_mode = MGX_TOWER_REFERENCE;
    o->device = -1;          // current device
    o->coarse_tol = 1e-5;    // multigrid.cpp:60
    o->coarse_maxit = 1000;  // multigrid.cpp:60
    o->max_cycle = 50;       // multigrid.cpp:94
    o->smoother = 0;
    o->fuse = 3;
    o->fp_mode = MGX_FP_BITWISE;
}

// ---- gs.h mirror (reference layout, device pointers, null stream)
int mgx_gauss_seidel(double *u, const double *rhs, long n, const double *v1, const double *v2,
                     double k, double nu, double h) {
    if (!u || !rhs || !v1 || !v2 || n < 2) return fail(MGX_E_ARG, "mgx_gauss_seidel: bad args");
    mgx::Coef c = mgx::make_coef(k, nu, h);
    mgx::launch_raw_gs_colour(u, rhs, v1, v2, n, c, 0, nullptr);
    mgx::launch_raw_gs_colour(u, rhs, v1, v2, n, c, 1, nullptr);
    return check_launch("mgx_gauss_seidel");
}
int mgx_residual(double *res, const double *u, const double *rhs, long n, const double *v1,
                 const double *v2, double k, double nu, double h) {
    if (!res || !u || !rhs || !v1 || !v2 || n < 2) return fail(MGX_E_ARG, "mgx_residual: bad args");
    mgx::launch_raw_residual(res, u, rhs, v1, v2, n, mgx::make_coef(k, nu, h), nullptr);
    return check_launch("mgx_residual");
}
int mgx_compute_norm(const double *res, long n, double *norm) {
    if (!res || !norm || n < 1) return fail(MGX_E_ARG, "mgx_compute_norm: bad args");
    std::lock_guard<std::mutex> g(g_raw_mu);
    double *s = nullptr;
    CHK(raw_scratch(&s));
    double *out = s + mgx::norm_partials_size();
    mgx::launch_norm(res, n, n + 1, s, out, nullptr);
    CHK(check_launch("mgx_compute_norm"));
    HIPCHK(hipMemcpy(norm, out, sizeof(double), hipMemcpyDeviceToHost));
    return MGX_OK;
}
int mgx_prolongation(double *up, const double *u, long n) {
    if (!up || !u || n < 1) return fail(MGX_E_ARG, "mgx_prolongation: bad args");
    mgx::launch_raw_prolongation(up, u, n, nullptr);
    return check_launch("mgx_prolongation");
}
int mgx_restriction(double *u, const double *up, long n) {
    if (!u || !up || n < 2) return fail(MGX_E_ARG, "mgx_restriction: bad args");
    mgx::launch_injection(u, n / 2 + 1, up, n + 1, n / 2 + 1, nullptr);
    return check_launch("mgx_restriction");
}
int mgx_compute_rhs(double *rhs, const double *u, long n, const double *v1, const double *v2,
                    double k, double nu, double h) {
    if (!rhs || !u || !v1 || !v2 || n < 2) return fail(MGX_E_ARG, "mgx_compute_rhs: bad args");
    mgx::launch_raw_rhs(rhs, u, v1, v2, n, mgx::make_coef(k, nu, h), nullptr);
    return check_launch("mgx_compute_rhs");
}

}  // extern "C"

// ---- context
int mgxi::create_ctx(mgx_ctx **out, long n, int maxlvl, double dt, double nu,
                     const mgx_options *opt, hipStream_t borrowed) {
    if (!out) return fail(MGX_E_ARG, "mgx_create: null out");
    *out = nullptr;
    if (!is_pow2(n)) return fail(MGX_E_ARG, "mgx_create: n must be a power of two >= 2");
    if (maxlvl < 1 || (n >> (maxlvl - 1)) < 2)
        return fail(MGX_E_ARG, "mgx_create: maxlvl must satisfy 1 <= maxlvl, n>>(maxlvl-1) >= 2");
    mgx_options o;
    mgx_default_options(&o);
    if (opt) o = *opt;
    if (o.fuse < 1 || o.fuse > mgx::kSmoothMaxSweeps) o.fuse = mgx::kSmoothMaxSweeps;
    if (o.nsmooth < 0 || o.shape < 1 || o.coarse_maxit < 1 || o.max_cycle < 1 ||
        o.smoother < 0 || o.smoother > 2 || (o.fp_mode != MGX_FP_BITWISE && o.fp_mode != MGX_FP_FMA))
        return fail(MGX_E_ARG, "mgx_create: bad options");
    mgx_ctx *c = new mgx_ctx();
    c->N = n;
    c->L = maxlvl;
    c->dt = dt;
    c->nu = nu;
    c->opt = o;
    auto bail = [&](int rc) {
        free_ctx(c);
        return rc;
    };
    if (o.device >= 0) {
        hipError_t e = hipSetDevice(o.device);
        if (e != hipSuccess) return bail(fail(MGX_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e)));
    }
    if (hipGetDevice(&c->device) != hipSuccess) return bail(fail(MGX_E_HIP, "hipGetDevice"));
    if (borrowed) {
        c->stream = borrowed;
        c->own_stream = false;
    } else if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        return bail(fail(MGX_E_HIP, "hipStreamCreate"));
    }
    c->lv.resize(maxlvl);
    double h = 1.0 / n;   // dx (multigrid.cpp:194), doubled per level (:49)
    for (int l = 0; l < maxlvl; ++l) {
        Level &L = c->lv[l];
        L.n = n >> l;
        L.pitch = mgx::tower_pitch(L.n);
        L.coef = mgx::make_coef(dt, nu, h, o.fp_mode == MGX_FP_FMA);
        L.coef_rhs = L.coef;   // theta = 1/2 until mgx_set_time_step
        h = 2 * h;
        const size_t bytes = sizeof(double) * L.pitch * (L.n + 1);
        double **bufs[5] = {&L.u[0], &L.u[1], &L.rhs, &L.v1, &L.v2};
        for (double **b : bufs) {
            if (hipMalloc(b, bytes) != hipSuccess)
                return bail(fail(MGX_E_HIP, "hipMalloc (level tower): out of device memory"));
            if (hipMemsetAsync(*b, 0, bytes, c->stream) != hipSuccess)
                return bail(fail(MGX_E_HIP, "hipMemset"));
        }
    }
    if (maxlvl >= 3 && c->lv[maxlvl - 1].n <= mgx::kCoarseLdsMaxN) {
        // coarsest level: the second rhs of a W-cycle pair pass with the fused
        // solve (op_wpair); zero boundary, as the restriction writes the interior
        Level &L = c->lv[maxlvl - 1];
        const size_t bytes = sizeof(double) * L.pitch * (L.n + 1);
        if (hipMalloc(&L.rhs_alt, bytes) != hipSuccess ||
            hipMemsetAsync(L.rhs_alt, 0, bytes, c->stream) != hipSuccess)
            return bail(fail(MGX_E_HIP, "hipMalloc (coarsest rhs)"));
    }
    if (maxlvl > 1 && n >= kCrossMinN) {   // third finest-level buffer: cross-cycle pass
        Level &L = c->lv[0];
        const size_t bytes = sizeof(double) * L.pitch * (L.n + 1);
        if (hipMalloc(&L.u[2], bytes) != hipSuccess)
            return bail(fail(MGX_E_HIP, "hipMalloc (level tower): out of device memory"));
    }
    const size_t flat = sizeof(double) * (n + 1) * (n + 1);
    // (two partial arrays: the cross pass's time-step mode sums two norms)
    if (hipMalloc(&c->zrow, sizeof(double) * c->lv[0].pitch) != hipSuccess ||
        hipMemsetAsync(c->zrow, 0, sizeof(double) * c->lv[0].pitch, c->stream) != hipSuccess)
        return bail(fail(MGX_E_HIP, "hipMalloc (zero row)"));
    if (hipMalloc(&c->partials, 2 * sizeof(double) * mgx::norm_partials_size()) != hipSuccess ||
        hipMalloc(&c->dscal, sizeof(double) * 8) != hipSuccess ||
        hipHostMalloc(&c->hscal, sizeof(double) * 8) != hipSuccess)
        return bail(fail(MGX_E_HIP, "hipMalloc (scratch)"));
    if (maxlvl > 1 && o.tower_mode == MGX_TOWER_REFERENCE) {
        if (hipMalloc(&c->stage[0], flat) != hipSuccess || hipMalloc(&c->stage[1], flat) != hipSuccess)
            return bail(fail(MGX_E_HIP, "hipMalloc (staging)"));
    }
    (void)hipMemsetAsync(c->dscal, 0, sizeof(double) * 8, c->stream);
    memset(c->hscal, 0, sizeof(double) * 8);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return bail(fail(MGX_E_HIP, "sync"));
    *out = c;
    return MGX_OK;
}

extern "C" {

int mgx_create(mgx_ctx **out, long n, int maxlvl, double dt, double nu, const mgx_options *opt) {
    return create_ctx(out, n, maxlvl, dt, nu, opt, nullptr);
}

int mgx_destroy(mgx_ctx *c) {
    free_ctx(c);
    return MGX_OK;
}

}  // extern "C"

// Everything derived from the finest v1 / v2 (already copied into level 0, or
// being copied on the stream): the coarse tower, its zero rows, the finest
// factors and the generating levels.  v1 / v2: the caller's arrays (host
// pointers for hipMemcpyHostToDevice).  Captured sub-cycles hold the old
// velocity's vz / vgen / factor pointers in their kernel arguments, so they go.
static int derive_velocity(mgx_ctx *c, const double *v1, const double *v2, hipMemcpyKind kind) {
    Level &L = c->lv[0];
    // (a replay may still be running: free_ctx drains the stream first too)
    if (!c->graphs.empty()) HIPCHK(hipStreamSynchronize(c->stream));
    free_graphs(c);
    CHK(build_tower(c));
    CHK(find_zero_rows(c));
    // exact velocity factors for the finest level's cross pass: from the host
    // arrays, or from the tower copy on the device ("device_factor")
    free_level_factors(L);
    std::vector<double> a1, b1, a2, b2;
    const bool host = kind == hipMemcpyHostToDevice;
    bool found = false;
    if (c->L > 1 && c->N >= kCrossMinN) {
        if (host ? g_device_factor == 2 : g_device_factor >= 1)
            CHK(factor_velocity_device(c, L.coef.h * 0.5, a1, b1, a2, b2, &found));
        else if (host)
            found = factor_velocity(v1, v2, c->N, 0, c->N + 1, L.coef.h * 0.5, a1, b1, a2, b2);
    }
    if (found) CHK(set_level_factors(L, 0, a1, b1, a2, b2, c->stream));
    CHK(find_vgen(c, a1, a2));
    return MGX_OK;
}

int mgxi::upload_ctx(mgx_ctx *c, const double *u0, const double *v1, const double *v2,
                     hipMemcpyKind kind) {
    if (!c || !u0 || !v1 || !v2) return fail(MGX_E_ARG, "mgx_upload: bad args");
    HIPCHK(hipSetDevice(c->device));
    Level &L = c->lv[0];
    const size_t row = (c->N + 1) * sizeof(double);
    L.cur = 0;
    L.zero = false;
    L.spec = -1;
    L.xin = -1;
    L.packed[0] = L.packed[1] = L.packed[2] = false;
    c->step_spec = false;   // a pending next-step state belongs to the old fields
    const double *src[3] = {u0, v1, v2};
    double *dst[3] = {L.u[0], L.v1, L.v2};
    for (int k = 0; k < 3; ++k)
        HIPCHK(hipMemcpy2DAsync(dst[k], L.pitch * sizeof(double), src[k], row, row, c->N + 1,
                                kind, c->stream));
    for (int l = 1; l < c->L; ++l) {
        c->lv[l].cur = 0;
        c->lv[l].zero = false;
    }
    CHK(derive_velocity(c, v1, v2, kind));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MGX_OK;
}

// mgx_set_velocity: the finest u stays where it is (the buffer mgx_download
// reads); everything computed with the old velocity is dropped.
static int set_velocity_impl(mgx_ctx *c, const double *v1, const double *v2,
                             hipMemcpyKind kind) {
    if (!c || !v1 || !v2) return fail(MGX_E_ARG, "mgx_set_velocity: bad args");
    if (c->dist)
        return fail(MGX_E_ARG, "mgx_set_velocity: not available on a partitioned context "
                               "(upload the new fields with mgx_upload)");
    HIPCHK(hipSetDevice(c->device));
    CHK(materialize(c, 0));
    Level &L = c->lv[0];
    // the speculative next cycle / next step, the unstored u_post's input, a
    // deferred coarsest solve: all formed with the old velocity
    L.spec = -1;
    L.xin = -1;
    L.packed[0] = L.packed[1] = L.packed[2] = false;
    c->step_spec = false;
    c->step_next = false;
    c->step_res0 = 0;
    c->post_only = false;
    c->cf_level = -1;
    c->cf_reps = 0;
    const size_t row = (c->N + 1) * sizeof(double);
    const double *src[2] = {v1, v2};
    double *dst[2] = {L.v1, L.v2};
    for (int k = 0; k < 2; ++k)
        HIPCHK(hipMemcpy2DAsync(dst[k], L.pitch * sizeof(double), src[k], row, row, c->N + 1,
                                kind, c->stream));
    for (int l = 1; l < c->L; ++l) {
        c->lv[l].cur = 0;
        c->lv[l].zero = false;
    }
    CHK(derive_velocity(c, v1, v2, kind));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MGX_OK;
}

// Whatever was formed from the old right-hand side goes: the speculative next
// cycle / next step (made with the old rhs), the unstored u_post's input.  The
// finest u stays where it is, as in set_velocity_impl.
void mgxi::drop_source_state(mgx_ctx *c) {
    drop_spec(c);
    if (!c->lv.empty()) c->lv[0].xin = -1;
    c->step_next = false;
    c->step_res0 = 0;
    c->post_only = false;
}

// mgx_set_source on a single-GPU context: the context's own pitched copy of f
// (allocated on the first call, reused by a replacement), or none.
int mgxi::set_source_ctx(mgx_ctx *c, const double *f, hipMemcpyKind kind) {
    HIPCHK(hipSetDevice(c->device));
    drop_source_state(c);
    Level &L = c->lv[0];
    if (c->src_terms) {   // one source per context: the separable one goes
        HIPCHK(hipStreamSynchronize(c->stream));   // a pass may still read the factors
        (void)hipFree(c->src_a);
        (void)hipFree(c->src_b);
        c->src_a = c->src_b = nullptr;
        c->src_terms = 0;
        c->src_active = false;
    }
    if (!f) {
        if (c->src) {
            HIPCHK(hipStreamSynchronize(c->stream));   // a pass may still read it
            (void)hipFree(c->src);
            c->src = nullptr;
        }
        c->src_active = false;
        return MGX_OK;
    }
    const size_t bytes = sizeof(double) * (size_t)(L.n + 1) * (size_t)L.pitch;
    if (!c->src) {
        const hipError_t e = hipMalloc(&c->src, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            c->src = nullptr;
            c->src_active = false;
            return fail(MGX_E_HIP, std::string("mgx_set_source: no room for the context's copy "
                                               "of the source (one finest-level array): ") +
                                       hipGetErrorString(e));
        }
        // (the pad columns are never read past column n; zero all the same)
        HIPCHK(hipMemsetAsync(c->src, 0, bytes, c->stream));
    }
    const size_t row = (c->N + 1) * sizeof(double);
    HIPCHK(hipMemcpy2DAsync(c->src, L.pitch * sizeof(double), f, row, row, c->N + 1, kind,
                            c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // the caller's buffer is free on return
    c->src_active = true;
    return MGX_OK;
}

// The device copies of separable factors: a -> terms rows of n+1, b -> terms
// rows of `pitch` (the pad zeroed once, at allocation; the copies write n+1
// entries per row).  Both buffers are sized for MGX_SOURCE_MAX_TERMS, so a
// replacement with another term count reuses them.
int mgxi::copy_source_factors(double **da, double **db, long n, long pitch, int terms,
                              const double *a, const double *b, hipMemcpyKind kind,
                              hipStream_t s, const char *who) {
    const size_t abytes = sizeof(double) * (size_t)MGX_SOURCE_MAX_TERMS * (size_t)(n + 1);
    const size_t bbytes = sizeof(double) * (size_t)MGX_SOURCE_MAX_TERMS * (size_t)pitch;
    double **dst[2] = {da, db};
    const size_t bytes[2] = {abytes, bbytes};
    for (int k = 0; k < 2; ++k) {
        if (*dst[k]) continue;
        const hipError_t e = hipMalloc(dst[k], bytes[k]);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            *dst[k] = nullptr;
            return fail(MGX_E_HIP, std::string(who) + ": no room for the factors: " +
                                       hipGetErrorString(e));
        }
        HIPCHK(hipMemsetAsync(*dst[k], 0, bytes[k], s));
    }
    const size_t row = (size_t)(n + 1) * sizeof(double);
    HIPCHK(hipMemcpyAsync(*da, a, row * terms, kind, s));
    HIPCHK(hipMemcpy2DAsync(*db, pitch * sizeof(double), b, row, row, terms, kind, s));
    return MGX_OK;
}

// mgx_set_source_separable on a single-GPU context: no finest-level array
int mgxi::set_source_sep_ctx(mgx_ctx *c, int terms, const double *a, const double *b,
                             hipMemcpyKind kind) {
    HIPCHK(hipSetDevice(c->device));
    drop_source_state(c);
    Level &L = c->lv[0];
    if (c->src) {   // one source per context: the field copy goes
        HIPCHK(hipStreamSynchronize(c->stream));   // a pass may still read it
        (void)hipFree(c->src);
        c->src = nullptr;
    }
    const int rc = copy_source_factors(&c->src_a, &c->src_b, L.n, L.pitch, terms, a, b, kind,
                                       c->stream, "mgx_set_source_separable");
    if (rc != MGX_OK || hipStreamSynchronize(c->stream) != hipSuccess) {
        (void)hipGetLastError();
        c->src_terms = 0;
        c->src_active = false;
        return rc != MGX_OK ? rc : fail(MGX_E_HIP, "mgx_set_source_separable: copy");
    }
    c->src_terms = terms;   // (the caller's buffers are free on return)
    c->src_active = true;
    return MGX_OK;
}

static int set_source_sep_impl(mgx_ctx *c, int terms, const double *a, const double *b,
                               hipMemcpyKind kind, const char *who) {
    if (!c) return fail(MGX_E_ARG, std::string(who) + ": null ctx");
    if (terms < 1 || terms > MGX_SOURCE_MAX_TERMS)
        return fail(MGX_E_ARG, std::string(who) + ": terms must be 1.." +
                                   std::to_string(MGX_SOURCE_MAX_TERMS));
    if (!a || !b) return fail(MGX_E_ARG, std::string(who) + ": null factors");
    if (c->dist) return dist_set_source_sep(c, terms, a, b, kind);
    return set_source_sep_ctx(c, terms, a, b, kind);
}

static int set_source_rows_impl(mgx_ctx *c, const double *const *f, hipMemcpyKind kind,
                                const char *who) {
    if (!c) return fail(MGX_E_ARG, std::string(who) + ": null ctx");
    if (!f) return fail(MGX_E_ARG, std::string(who) + ": null block list");
    const int parts = c->dist ? dist_nsub(c) : 1;
    for (int i = 0; i < parts; ++i)
        if (!f[i]) return fail(MGX_E_ARG, std::string(who) + ": null block");
    if (c->dist) {
        if (dist_la(c) == 0)
            return fail(MGX_E_ARG, std::string(who) + ": no partitioned level, use mgx_set_source");
        return dist_set_source_rows(c, f, kind);
    }
    return set_source_ctx(c, f[0], kind);   // part 0 is all rows
}

static int set_source_impl(mgx_ctx *c, const double *f, hipMemcpyKind kind, const char *who) {
    if (!c) return fail(MGX_E_ARG, std::string(who) + ": null ctx");
    if (c->dist) return dist_set_source(c, f, kind);
    return set_source_ctx(c, f, kind);
}

extern "C" {

int mgx_set_source(mgx_ctx *c, const double *f) {
    return set_source_impl(c, f, hipMemcpyHostToDevice, "mgx_set_source");
}
int mgx_set_source_device(mgx_ctx *c, const double *f) {
    return set_source_impl(c, f, hipMemcpyDeviceToDevice, "mgx_set_source_device");
}
int mgx_set_source_scale(mgx_ctx *c, double s) {
    if (!c) return fail(MGX_E_ARG, "mgx_set_source_scale: null ctx");
    if (c->dist) {
        HIPCHK(hipSetDevice(c->device));
        dist_set_source_scale(c, s);
    } else {
        drop_source_state(c);
    }
    c->src_scale = s;
    return MGX_OK;
}
int mgx_source_info(mgx_ctx *c, int *active, double *scale) {
    if (!c) return fail(MGX_E_ARG, "mgx_source_info: null ctx");
    if (active) *active = c->src_active ? 1 : 0;
    if (scale) *scale = c->src_scale;
    return MGX_OK;
}
int mgx_set_source_separable(mgx_ctx *c, int terms, const double *a, const double *b) {
    return set_source_sep_impl(c, terms, a, b, hipMemcpyHostToDevice, "mgx_set_source_separable");
}
int mgx_set_source_separable_device(mgx_ctx *c, int terms, const double *a, const double *b) {
    return set_source_sep_impl(c, terms, a, b, hipMemcpyDeviceToDevice,
                               "mgx_set_source_separable_device");
}
int mgx_set_source_rows(mgx_ctx *c, const double *const *f) {
    return set_source_rows_impl(c, f, hipMemcpyHostToDevice, "mgx_set_source_rows");
}
int mgx_set_source_rows_device(mgx_ctx *c, const double *const *f) {
    return set_source_rows_impl(c, f, hipMemcpyDeviceToDevice, "mgx_set_source_rows_device");
}
int mgx_source_kind(mgx_ctx *c, int *kind, int *terms) {
    if (!c) return fail(MGX_E_ARG, "mgx_source_kind: null ctx");
    if (kind) *kind = !c->src_active ? 0 : c->src_terms ? 2 : 1;
    if (terms) *terms = c->src_active ? c->src_terms : 0;
    return MGX_OK;
}
int mgx_compute_rhs_source_separable(double *rhs, const double *u, long n, const double *v1,
                                     const double *v2, double k, double nu, double h, int terms,
                                     const double *a, const double *b, double cf) {
    if (!rhs || !u || !v1 || !v2 || !a || !b)
        return fail(MGX_E_ARG, "mgx_compute_rhs_source_separable: null pointer");
    if (n < 2) return fail(MGX_E_ARG, "mgx_compute_rhs_source_separable: n must be >= 2");
    if (terms < 1 || terms > MGX_SOURCE_MAX_TERMS)
        return fail(MGX_E_ARG, "mgx_compute_rhs_source_separable: terms must be 1.." +
                                   std::to_string(MGX_SOURCE_MAX_TERMS));
    mgxsrc::launch_raw_rhs_source_sep(rhs, u, v1, v2, terms, a, b, cf, n,
                                      mgx::make_coef(k, nu, h), nullptr);
    return check_launch("mgx_compute_rhs_source_separable");
}
int mgx_compute_rhs_source(double *rhs, const double *u, long n, const double *v1,
                           const double *v2, double k, double nu, double h, const double *f,
                           double cf) {
    if (!rhs || !u || !v1 || !v2 || !f || n < 2)
        return fail(MGX_E_ARG, "mgx_compute_rhs_source: bad args");
    mgxsrc::launch_raw_rhs_source(rhs, u, v1, v2, f, cf, n, mgx::make_coef(k, nu, h), nullptr);
    return check_launch("mgx_compute_rhs_source");
}

// (a pending ring, mgx_set_boundary(MGX_BC_NEXT_STEP), belongs to the old u:
// every upload cancels it)
int mgx_upload(mgx_ctx *c, const double *u0, const double *v1, const double *v2) {
    if (c) c->bc_pending = false;
    if (c) c->hist_invalidate();   // (a history belongs to the old u too)
    if (c && c->dist) return dist_upload(c, u0, v1, v2, hipMemcpyHostToDevice);
    return upload_ctx(c, u0, v1, v2, hipMemcpyHostToDevice);
}
int mgx_upload_device(mgx_ctx *c, const double *u0, const double *v1, const double *v2) {
    if (c) c->bc_pending = false;
    if (c) c->hist_invalidate();
    if (c && c->dist) return dist_upload(c, u0, v1, v2, hipMemcpyDeviceToDevice);
    return upload_ctx(c, u0, v1, v2, hipMemcpyDeviceToDevice);
}
int mgx_set_velocity(mgx_ctx *c, const double *v1, const double *v2) {
    return set_velocity_impl(c, v1, v2, hipMemcpyHostToDevice);
}
int mgx_set_velocity_device(mgx_ctx *c, const double *v1, const double *v2) {
    return set_velocity_impl(c, v1, v2, hipMemcpyDeviceToDevice);
}

static int download_impl(mgx_ctx *c, int level, int field, double *out, hipMemcpyKind kind) {
    if (!c || !out || level < 0 || level >= c->L || field < 0 || field > 3)
        return fail(MGX_E_ARG, "mgx_download: bad args");
    HIPCHK(hipSetDevice(c->device));
    CHK(materialize(c, level));
    if (level == 0 && field == 0) CHK(op_expand(c));   // (a cycle that failed half-way)
    Level &L = c->lv[level];
    const double *src = field == 0 ? L.U() : field == 1 ? L.rhs : field == 2 ? L.v1 : L.v2;
    const size_t row = (L.n + 1) * sizeof(double);
    HIPCHK(hipMemcpy2DAsync(out, row, src, L.pitch * sizeof(double), row, L.n + 1, kind,
                            c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MGX_OK;
}

int mgx_download(mgx_ctx *c, double *u) {
    if (c && c->dist) return dist_download(c, u, hipMemcpyDeviceToHost);
    return download_impl(c, 0, 0, u, hipMemcpyDeviceToHost);
}
int mgx_download_device(mgx_ctx *c, double *u) {
    if (c && c->dist) return dist_download(c, u, hipMemcpyDeviceToDevice);
    return download_impl(c, 0, 0, u, hipMemcpyDeviceToDevice);
}
int mgx_download_level(mgx_ctx *c, int level, int field, double *out) {
    if (c && c->dist) return fail(MGX_E_ARG, "mgx_download_level: not available on a partitioned context");
    return download_impl(c, level, field, out, hipMemcpyDeviceToHost);
}
int mgx_owned_rows(mgx_ctx *c, int part, int *ra, int *rb) {
    if (!c || !ra || !rb) return fail(MGX_E_ARG, "mgx_owned_rows: bad args");
    if (c->dist) return dist_owned_rows(c, part, ra, rb);
    if (part != 0) return fail(MGX_E_ARG, "mgx_owned_rows: a single-GPU context has part 0 only");
    *ra = 0;
    *rb = (int)c->N + 1;
    return MGX_OK;
}
int mgx_download_rows(mgx_ctx *c, int part, double *rows) {
    if (!c || !rows) return fail(MGX_E_ARG, "mgx_download_rows: bad args");
    if (c->dist) return dist_download_rows(c, part, rows, hipMemcpyDeviceToHost);
    if (part != 0) return fail(MGX_E_ARG, "mgx_download_rows: a single-GPU context has part 0 only");
    return download_impl(c, 0, 0, rows, hipMemcpyDeviceToHost);
}

}  // extern "C"

// ---- field diagnostics (include/mgx.h "Field diagnostics", csrc/diag.hip)
// The context's scratch (partial records + one result record), allocated by
// the first statistics call: a context that never asks keeps no byte of it.
static int diag_scratch(mgx_ctx *c, mgxdiag::Rec **p) {
    if (!c->diag) HIPCHK(hipMalloc(&c->diag, mgxdiag::scratch_bytes(1)));
    *p = static_cast<mgxdiag::Rec *>(c->diag);
    return MGX_OK;
}
static void window(long n, long r0, long r1, int interior, long *ra, long *rb, long *j0,
                   long *j1) {
    *ra = interior ? std::max<long>(r0, 1) : r0;
    *rb = interior ? std::min<long>(r1, n) : r1;
    *j0 = interior ? 1 : 0;
    *j1 = interior ? n - 1 : n;
}
int mgxi::stats_view(mgx_ctx *c, const mgxdiag::View &f, long r0, long r1, int interior,
                     const double *minus, long minus_row0, mgx_stats *out) {
    if (f.n + 1 > 512L * 4096) return fail(MGX_E_ARG, "mgx_field_stats: level too wide");
    mgxdiag::Rec *scr = nullptr;
    CHK(diag_scratch(c, &scr));
    mgxdiag::StatsArgs A;
    A.f = f;
    A.minus = minus;
    A.minus_row0 = minus_row0;
    window(f.n, r0, r1, interior, &A.r0, &A.r1, &A.j0, &A.j1);
    A.partials = scr;
    A.out = scr + mgxdiag::kMaxPartials;
    mgxdiag::PassTimer T;
    T.begin(c->stream);
    mgxdiag::launch_stats(A, c->stream);
    T.end(c->stream);
    CHK(check_launch("field statistics"));
    mgxdiag::Rec h;
    HIPCHK(hipMemcpyAsync(&h, A.out, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    mgxdiag::to_stats(h, f.n, A.r0, A.r1, A.j0, A.j1, out);
    T.commit(8.0 * (double)out->count * (minus ? 2.0 : 1.0));
    return MGX_OK;
}
int mgxi::sample_pieces(mgx_ctx *c, const std::vector<SamplePiece> &pieces, long stride, long A0,
                        long rows, double *out, bool device_out) {
    if (rows <= 0) return MGX_OK;
    const long cols = pieces[0].f.n / stride + 1;
    double *dst = out;
    if (!device_out) HIPCHK(hipMalloc(&dst, sizeof(double) * (size_t)rows * (size_t)cols));
    int rc = MGX_OK;
    for (const SamplePiece &p : pieces) {
        mgxdiag::launch_gather(p.f, stride, p.A0, p.A1, dst + (p.A0 - A0) * cols, cols, c->stream);
        if ((rc = check_launch("field sample")) != MGX_OK) break;
    }
    if (rc == MGX_OK && !device_out &&
        hipMemcpyAsync(out, dst, sizeof(double) * (size_t)rows * (size_t)cols,
                       hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = fail(MGX_E_HIP, "field sample: copy");
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == MGX_OK)
        rc = fail(MGX_E_HIP, "field sample: sync");
    if (!device_out) (void)hipFree(dst);
    return rc;
}
// fields 5 and 6, the history arrays h and h2 (level 0, and only while they
// hold a time level): host-only, the flags of the context that owns them
int mgxi::history_field_check(const mgx_ctx *c, int level, int field, const char *who) {
    if (field != 5 && field != 6) return MGX_OK;
    if (level != 0)
        return fail(MGX_E_ARG, std::string(who) + ": the history is a finest-level array (fields "
                                                  "5 and 6, level 0)");
    if (field == 5 && !(c->hist_on && c->hist_valid))
        return fail(MGX_E_ARG, std::string(who) + ": no valid history (field 5: "
                                                  "mgx_set_history, then a step)");
    if (field == 6 && !(c->hist2_on && c->hist2_valid))
        return fail(MGX_E_ARG, std::string(who) + ": no valid second history array (field 6: "
                                                  "mgx_set_history_depth(ctx, 2), then two steps)");
    return MGX_OK;
}
// host-only argument check of (level, field) on a single-GPU context
static int field_check(mgx_ctx *c, int level, int field, const char *who) {
    if (level < 0 || level >= c->L)
        return fail(MGX_E_ARG, std::string(who) + ": level out of range");
    if (field < 0 || field > 6)
        return fail(MGX_E_ARG, std::string(who) + ": field must be 0..6 (u, rhs, v1, v2, source, "
                                                  "history, history2)");
    CHK(history_field_check(c, level, field, who));
    if (field == 4 && level == 0 && c->src_terms)
        return fail(MGX_E_ARG, std::string(who) + ": the source is separable: no copy of it is "
                                                  "kept (field 4)");
    if (field == 4 && (level != 0 || !c->src))
        return fail(MGX_E_ARG, std::string(who) + ": no source is set (field 4 is the context's "
                                                  "copy of it, level 0)");
    return MGX_OK;
}
// what mgx_download_level(level, field) copies: the same materialize + U() route
int mgxi::field_view(mgx_ctx *c, int level, int field, mgxdiag::View *v) {
    HIPCHK(hipSetDevice(c->device));
    CHK(materialize(c, level));
    Level &L = c->lv[level];
    v->a = field == 0 ? L.U() : field == 1 ? L.rhs : field == 2 ? L.v1 : field == 3 ? L.v2
         : field == 4 ? c->src : field == 5 ? c->hist : c->hist2;
    v->row0 = 0;
    v->pitch = L.pitch;
    v->n = L.n;
    return MGX_OK;
}

extern "C" {

int mgx_stats_merge(mgx_stats *into, const mgx_stats *other) {
    if (!into || !other) return fail(MGX_E_ARG, "mgx_stats_merge: null argument");
    mgxdiag::merge(into, *other);
    return MGX_OK;
}
int mgx_array_stats(const double *a, const double *minus, long n, int interior_only,
                    mgx_stats *out) {
    if (!a || !out || n < 1) return fail(MGX_E_ARG, "mgx_array_stats: bad args");
    std::lock_guard<std::mutex> g(g_raw_mu);
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    static mgxdiag::Rec *scr = nullptr;
    static int scr_dev = -1;
    if (!scr || scr_dev != dev) {
        HIPCHK(hipMalloc(&scr, mgxdiag::scratch_bytes(1)));
        scr_dev = dev;
    }
    long r0, r1, j0, j1;
    window(n, 0, n + 1, interior_only, &r0, &r1, &j0, &j1);
    mgxdiag::timer_reset();
    mgxdiag::PassTimer T;
    T.begin(nullptr);
    const bool ok = mgxdiag::launch_raw_stats(a, minus, n, r0, r1, j0, j1, scr,
                                              scr + mgxdiag::kMaxPartials, nullptr);
    T.end(nullptr);
    if (!ok) return fail(MGX_E_ARG, "mgx_array_stats: n too large");
    CHK(check_launch("mgx_array_stats"));
    mgxdiag::Rec h;
    HIPCHK(hipMemcpy(&h, scr + mgxdiag::kMaxPartials, sizeof(h), hipMemcpyDeviceToHost));
    mgxdiag::to_stats(h, n, r0, r1, j0, j1, out);
    T.commit(8.0 * (double)out->count * (minus ? 2.0 : 1.0));
    return MGX_OK;
}
int mgx_field_stats(mgx_ctx *c, int level, int field, int interior_only, const double *minus,
                    mgx_stats *out) {
    if (!c || !out) return fail(MGX_E_ARG, "mgx_field_stats: null argument");
    if (c->dist) return dist_field_stats(c, level, field, interior_only, minus, out);
    CHK(field_check(c, level, field, "mgx_field_stats"));
    mgxdiag::timer_reset();
    mgxdiag::View v;
    CHK(field_view(c, level, field, &v));
    return stats_view(c, v, 0, v.n + 1, interior_only, minus, 0, out);
}
int mgx_field_stats_rows(mgx_ctx *c, int part, int field, int interior_only,
                         const double *minus_rows, mgx_stats *out) {
    if (!c || !out) return fail(MGX_E_ARG, "mgx_field_stats_rows: null argument");
    if (c->dist) {
        if (field == 4 && c->src_active && c->src_terms)
            return fail(MGX_E_ARG, "mgx_field_stats_rows: the source is separable: no copy of "
                                   "it is kept (field 4)");
        if (field == 4 && !c->src_active)
            return fail(MGX_E_ARG, "mgx_field_stats_rows: no source is set");
        mgxdiag::timer_reset();
        return dist_field_stats_rows(c, part, field, interior_only, minus_rows, -1, out,
                                     "mgx_field_stats_rows");
    }
    if (part != 0)
        return fail(MGX_E_ARG, "mgx_field_stats_rows: a single-GPU context has part 0 only");
    CHK(field_check(c, 0, field, "mgx_field_stats_rows"));
    mgxdiag::timer_reset();
    mgxdiag::View v;
    CHK(field_view(c, 0, field, &v));
    return stats_view(c, v, 0, v.n + 1, interior_only, minus_rows, 0, out);
}
static int stride_check(long n, long stride, const char *who) {
    if (stride < 1 || stride > n || n % stride)
        return fail(MGX_E_ARG, std::string(who) + ": stride must divide the level's n (1 <= "
                                                  "stride <= n)");
    return MGX_OK;
}
static int sample_impl(mgx_ctx *c, int level, int field, long stride, double *out,
                       bool device_out, const char *who) {
    if (stride < 1) return fail(MGX_E_ARG, std::string(who) + ": stride must be >= 1");
    if (!c || !out) return fail(MGX_E_ARG, std::string(who) + ": null argument");
    if (c->dist) return dist_sample(c, level, field, stride, out, device_out, who);
    CHK(field_check(c, level, field, who));
    CHK(stride_check(c->lv[level].n, stride, who));
    SamplePiece p;
    CHK(field_view(c, level, field, &p.f));
    p.A0 = 0;
    p.A1 = p.f.n / stride + 1;
    return sample_pieces(c, {p}, stride, 0, p.A1, out, device_out);
}
int mgx_sample(mgx_ctx *c, int level, int field, long stride, double *out) {
    return sample_impl(c, level, field, stride, out, false, "mgx_sample");
}
int mgx_sample_device(mgx_ctx *c, int level, int field, long stride, double *out) {
    return sample_impl(c, level, field, stride, out, true, "mgx_sample_device");
}
int mgx_sample_rows(mgx_ctx *c, int part, int field, long stride, double *out, long *first_row,
                    long *rows) {
    if (stride < 1) return fail(MGX_E_ARG, "mgx_sample_rows: stride must be >= 1");
    if (!c || !first_row || !rows) return fail(MGX_E_ARG, "mgx_sample_rows: null argument");
    if (c->dist) return dist_sample_rows(c, part, field, stride, out, first_row, rows);
    if (part != 0) return fail(MGX_E_ARG, "mgx_sample_rows: a single-GPU context has part 0 only");
    CHK(field_check(c, 0, field, "mgx_sample_rows"));
    CHK(stride_check(c->N, stride, "mgx_sample_rows"));
    *first_row = 0;
    *rows = c->N / stride + 1;
    if (!out) return MGX_OK;
    return sample_impl(c, 0, field, stride, out, false, "mgx_sample_rows");
}

}  // extern "C"

// ---- the step error estimate (include/mgx.h "Step error estimate", csrc/errest.hip)
int mgxi::step_error_view(mgx_ctx *c, const double *u, const double *h, const double *h2, long row0,
                          long pitch, long n, long r0, long r1, double w, double atol, double rtol,
                          mgx_step_err *out) {
    mgxdiag::Rec *scr = nullptr;
    CHK(diag_scratch(c, &scr));
    mgxerr::Args A;
    A.u = u;
    A.h = h;
    A.h2 = h2;
    A.row0 = row0;
    A.pitch = pitch;
    A.n = n;
    A.r0 = std::max<long>(r0, 1);   // the interior rows of [r0, r1)
    A.r1 = std::max<long>(A.r0, std::min<long>(r1, n));
    A.w = w;
    A.p = 1.0 + w;
    A.atol = atol;
    A.rtol = rtol;
    A.partials = reinterpret_cast<mgxerr::Rec *>(scr);
    A.out = A.partials + mgxdiag::kMaxPartials;
    mgxerr::PassTimer T;
    T.begin(c->stream);
    const bool ok = mgxerr::launch_step_error(A, c->stream);
    T.end(c->stream);
    if (!ok) return fail(MGX_E_ARG, "mgx_step_error: level too wide");
    CHK(check_launch("step error estimate"));
    mgxerr::Rec r;
    HIPCHK(hipMemcpyAsync(&r, A.out, sizeof(r), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    mgxerr::to_step_err(r, n, A.r0, A.r1, w, out);
    T.commit(24.0 * (double)out->count);
    return MGX_OK;
}
// host-only checks shared by mgx_step_error and mgx_step_error_rows
static int step_error_check(mgx_ctx *c, double atol, double rtol, mgx_step_err *out,
                            const char *who) {
    if (!c || !out) return fail(MGX_E_ARG, std::string(who) + ": null argument");
    if (!mgxerr::tolerances_ok(atol, rtol))
        return fail(MGX_E_ARG, std::string(who) + ": atol and rtol must be finite and >= 0, and "
                                                  "not both zero");
    if (!c->hist_on || !c->hist2_on)
        return fail(MGX_E_ARG, std::string(who) + ": the context has no history of depth 2 "
                                                  "(mgx_set_history_depth)");
    if (!c->hist_valid || !c->hist2_valid)
        return fail(MGX_E_ARG, std::string(who) + ": the history does not hold u^n and u^(n-1): "
                                                  "two steps since the last upload or rollback "
                                                  "give that");
    return MGX_OK;
}
// the single-GPU context's three arrays: u by the route mgx_field_stats takes
static int step_error_ctx(mgx_ctx *c, double w, double atol, double rtol, mgx_step_err *out) {
    mgxdiag::View v;
    CHK(field_view(c, 0, 0, &v));
    return step_error_view(c, v.a, c->hist, c->hist2, 0, v.pitch, v.n, 0, v.n + 1, w, atol, rtol,
                           out);
}

extern "C" {

int mgx_step_error(mgx_ctx *c, double atol, double rtol, mgx_step_err *out) {
    CHK(step_error_check(c, atol, rtol, out, "mgx_step_error"));
    const double w = c->hist_dt / c->hist2_dt;
    mgxerr::timer_reset();
    if (c->dist) return dist_step_error(c, w, atol, rtol, out);
    return step_error_ctx(c, w, atol, rtol, out);
}
int mgx_step_error_rows(mgx_ctx *c, int part, double atol, double rtol, mgx_step_err *out) {
    CHK(step_error_check(c, atol, rtol, out, "mgx_step_error_rows"));
    const double w = c->hist_dt / c->hist2_dt;
    mgxerr::timer_reset();
    if (c->dist) return dist_step_error_rows(c, part, w, atol, rtol, out, "mgx_step_error_rows");
    if (part != 0)
        return fail(MGX_E_ARG, "mgx_step_error_rows: a single-GPU context has part 0 only");
    return step_error_ctx(c, w, atol, rtol, out);
}
int mgx_step_err_merge(mgx_step_err *into, const mgx_step_err *other) {
    if (!into || !other) return fail(MGX_E_ARG, "mgx_step_err_merge: null argument");
    if (!mgxerr::merge(into, *other))
        return fail(MGX_E_ARG, "mgx_step_err_merge: the records' w differ: they are not of one "
                               "step");
    return MGX_OK;
}
int mgx_array_step_error(const double *u, const double *h, const double *h2, long n, double w,
                         double atol, double rtol, mgx_step_err *out) {
    if (!u || !h || !h2 || !out) return fail(MGX_E_ARG, "mgx_array_step_error: null argument");
    if (n < 2) return fail(MGX_E_ARG, "mgx_array_step_error: n must be >= 2");
    if (!mgxerr::tolerances_ok(atol, rtol))
        return fail(MGX_E_ARG, "mgx_array_step_error: atol and rtol must be finite and >= 0, and "
                               "not both zero");
    if (!std::isfinite(w))
        return fail(MGX_E_ARG, "mgx_array_step_error: w must be finite");
    std::lock_guard<std::mutex> g(g_raw_mu);
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    static mgxerr::Rec *scr = nullptr;
    static int scr_dev = -1;
    if (!scr || scr_dev != dev) {
        HIPCHK(hipMalloc(&scr, mgxdiag::scratch_bytes(1)));
        scr_dev = dev;
    }
    mgxerr::timer_reset();
    mgxerr::PassTimer T;
    T.begin(nullptr);
    const bool ok = mgxerr::launch_raw_step_error(u, h, h2, n, 1.0 + w, w, atol, rtol, scr,
                                                  scr + mgxdiag::kMaxPartials, nullptr);
    T.end(nullptr);
    if (!ok) return fail(MGX_E_ARG, "mgx_array_step_error: n too large");
    CHK(check_launch("mgx_array_step_error"));
    mgxerr::Rec r;
    HIPCHK(hipMemcpy(&r, scr + mgxdiag::kMaxPartials, sizeof(r), hipMemcpyDeviceToHost));
    mgxerr::to_step_err(r, n, 1, n, w, out);
    T.commit(24.0 * (double)out->count);
    return MGX_OK;
}

}  // extern "C"

// ---- dense output (include/mgx.h "Dense output", csrc/dense.hip)
// tuning key "dense_store": how the stride-1 march stores out (dense.h)
long mgxi::g_dense_store = 0;
// tuning key "dense_rows": the rows of a workgroup of that march (0: the row
// groups of the error pass; 4, one batch of loads, measured fastest: DESIGN 15)
long mgxi::g_dense_rows = 4;

int mgxi::dense_pieces(mgx_ctx *c, const std::vector<DensePiece> &pieces, long stride, long A0,
                       long rows, double *out, bool device_out) {
    if (rows <= 0) return MGX_OK;
    const long cols = pieces[0].s.n / stride + 1;
    const size_t bytes = sizeof(double) * (size_t)rows * (size_t)cols;
    double *dst = out;
    if (!device_out) HIPCHK(hipMalloc(&dst, bytes));
    int rc = MGX_OK;
    long pts = 0;
    mgxdense::PassTimer T;
    T.begin(c->stream);
    for (const DensePiece &p : pieces) {
        if (stride == 1)
            mgxdense::launch_march(p.s, p.A0, p.A1, dst, A0, (int)g_dense_store,
                                   (int)g_dense_rows, c->stream);
        else
            mgxdense::launch_gather(p.s, stride, p.A0, p.A1, dst + (p.A0 - A0) * cols, cols,
                                    c->stream);
        pts += std::max<long>(0, p.A1 - p.A0) * cols;
        if ((rc = check_launch("dense output")) != MGX_OK) break;
    }
    T.end(c->stream);
    if (rc == MGX_OK && !device_out &&
        hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = fail(MGX_E_HIP, "dense output: copy");
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == MGX_OK)
        rc = fail(MGX_E_HIP, "dense output: sync");
    if (!device_out) (void)hipFree(dst);
    if (rc == MGX_OK) T.commit(8.0 * (pieces[0].s.levels + 1) * (double)pts);
    return rc;
}
int mgxi::dense_points_pieces(mgx_ctx *c, const std::vector<DensePiece> &pieces, bool fill_unheld,
                              long npts, const long *pi, const long *pj, double *out) {
    mgxdense::PassTimer T;
    T.begin(c->stream);
    // (stream order: the first launch fills what no piece holds, the later ones
    // write their own rows only)
    for (size_t k = 0; k < pieces.size(); ++k) {
        const DensePiece &p = pieces[k];
        mgxdense::launch_points(p.s, p.A0, p.A1, fill_unheld && k == 0, npts, pi, pj, out,
                                c->stream);
        CHK(check_launch("dense points"));
    }
    T.end(c->stream);
    HIPCHK(hipStreamSynchronize(c->stream));
    T.commit(8.0 * (pieces[0].s.levels + 1) * (double)npts);
    return MGX_OK;
}
int mgxi::dense_src_ctx(mgx_ctx *c, int levels, const double w[3], mgxdense::Src *s) {
    mgxdiag::View v;
    CHK(field_view(c, 0, 0, &v));
    s->u = v.a;
    s->h = levels >= 2 ? c->hist : nullptr;
    s->h2 = levels >= 3 ? c->hist2 : nullptr;
    s->row0 = v.row0;
    s->pitch = v.pitch;
    s->n = v.n;
    s->levels = levels;
    s->w0 = w[0];
    s->w1 = w[1];
    s->w2 = w[2];
    return MGX_OK;
}
// host-only checks shared by the context's dense calls, and the weights from
// the history's own step sizes (not the context's current dt)
static int dense_check(mgx_ctx *c, int order, double tau, const char *who, double w[3]) {
    if (!c) return fail(MGX_E_ARG, std::string(who) + ": null ctx");
    if (order < 0 || order > 2)
        return fail(MGX_E_ARG, std::string(who) + ": order must be 0, 1 or 2");
    if (!std::isfinite(tau)) return fail(MGX_E_ARG, std::string(who) + ": tau must be finite");
    if (order >= 1 && !(c->hist_on && c->hist_valid))
        return fail(MGX_E_ARG, std::string(who) + ": order >= 1 needs a valid history "
                                                  "(mgx_set_history, then a step)");
    if (order == 2 && !(c->hist2_on && c->hist2_valid))
        return fail(MGX_E_ARG, std::string(who) + ": order 2 needs a history of depth 2 that holds "
                                                  "u^n and u^(n-1) (mgx_set_history_depth(ctx, "
                                                  "2), then two steps)");
    if (mgxdense::weights(order, tau, c->hist_dt, c->hist2_dt, w) != 0)
        return fail(MGX_E_ARG, std::string(who) + ": the history's step sizes are not positive");
    return MGX_OK;
}
static int dense_stride_check(long n, long stride, const char *who) {
    if (stride < 1 || stride > n || n % stride)
        return fail(MGX_E_ARG, std::string(who) + ": stride must divide N (1 <= stride <= N)");
    return MGX_OK;
}
static int dense_output_impl(mgx_ctx *c, int order, double tau, long stride, double *out,
                             bool device_out, const char *who) {
    double w[3];
    CHK(dense_check(c, order, tau, who, w));
    if (!out) return fail(MGX_E_ARG, std::string(who) + ": null out");
    CHK(dense_stride_check(c->N, stride, who));
    mgxdense::timer_reset();
    if (c->dist) return dist_dense(c, order + 1, w, stride, out, device_out, who);
    DensePiece p;
    CHK(dense_src_ctx(c, order + 1, w, &p.s));
    p.A0 = 0;
    p.A1 = c->N / stride + 1;
    return dense_pieces(c, {p}, stride, 0, p.A1, out, device_out);
}
// the context's staging of mgx_dense_points: room for npts points
static int dense_staging(mgx_ctx *c, long npts, long **pi, long **pj, double **val) {
    if (npts > c->dense_cap) {
        const long cap = std::max<long>(1024, std::max(npts, 2 * c->dense_cap));
        HIPCHK(hipStreamSynchronize(c->stream));
        (void)hipFree(c->dense_buf);
        c->dense_buf = nullptr;
        c->dense_cap = 0;
        HIPCHK(hipMalloc(&c->dense_buf, 24 * (size_t)cap));
        c->dense_cap = cap;
    }
    *pi = static_cast<long *>(c->dense_buf);
    *pj = *pi + c->dense_cap;
    *val = reinterpret_cast<double *>(*pj + c->dense_cap);
    return MGX_OK;
}
static int dense_points_launch(mgx_ctx *c, int levels, const double w[3], long npts,
                               const long *pi, const long *pj, double *out) {
    if (c->dist) return dist_dense_points(c, levels, w, npts, pi, pj, out);
    DensePiece p;
    CHK(dense_src_ctx(c, levels, w, &p.s));
    p.A0 = 0;
    p.A1 = c->N + 1;
    return dense_points_pieces(c, {p}, true, npts, pi, pj, out);
}

extern "C" {

int mgx_dense_weights(int order, double tau, double dt1, double dt2, double *w0, double *w1,
                      double *w2) {
    double w[3];
    switch (mgxdense::weights(order, tau, dt1, dt2, w)) {
    case 0: break;
    case 1: return fail(MGX_E_ARG, "mgx_dense_weights: order must be 0, 1 or 2");
    case 2: return fail(MGX_E_ARG, "mgx_dense_weights: tau must be finite");
    case 3: return fail(MGX_E_ARG, "mgx_dense_weights: dt1 must be finite and > 0 (order >= 1)");
    default: return fail(MGX_E_ARG, "mgx_dense_weights: dt2 must be finite and > 0 (order 2)");
    }
    if (w0) *w0 = w[0];
    if (w1) *w1 = w[1];
    if (w2) *w2 = w[2];
    return MGX_OK;
}
int mgx_dense_output(mgx_ctx *c, int order, double tau, long stride, double *out) {
    return dense_output_impl(c, order, tau, stride, out, false, "mgx_dense_output");
}
int mgx_dense_output_device(mgx_ctx *c, int order, double tau, long stride, double *out) {
    return dense_output_impl(c, order, tau, stride, out, true, "mgx_dense_output_device");
}
int mgx_dense_output_rows(mgx_ctx *c, int part, int order, double tau, long stride, double *out,
                          long *first_row, long *rows) {
    const char *who = "mgx_dense_output_rows";
    double w[3];
    CHK(dense_check(c, order, tau, who, w));
    if (!first_row || !rows) return fail(MGX_E_ARG, std::string(who) + ": null argument");
    CHK(dense_stride_check(c->N, stride, who));
    mgxdense::timer_reset();
    if (c->dist) return dist_dense_rows(c, part, order + 1, w, stride, out, first_row, rows, who);
    if (part != 0) return fail(MGX_E_ARG, std::string(who) + ": a single-GPU context has part 0 only");
    *first_row = 0;
    *rows = c->N / stride + 1;
    if (!out) return MGX_OK;
    DensePiece p;
    CHK(dense_src_ctx(c, order + 1, w, &p.s));
    p.A0 = 0;
    p.A1 = *rows;
    return dense_pieces(c, {p}, stride, 0, p.A1, out, false);
}
int mgx_dense_points(mgx_ctx *c, int order, double tau, long npts, const long *pi, const long *pj,
                     double *out) {
    const char *who = "mgx_dense_points";
    double w[3];
    CHK(dense_check(c, order, tau, who, w));
    if (npts < 0) return fail(MGX_E_ARG, std::string(who) + ": npts must be >= 0");
    if (npts > 0 && (!pi || !pj || !out))
        return fail(MGX_E_ARG, std::string(who) + ": null argument");
    mgxdense::timer_reset();
    if (npts == 0) return MGX_OK;
    // every index inside the grid, and in a row this context holds
    std::vector<std::pair<long, long>> held;
    if (c->dist) {
        for (int p = 0; p < dist_nsub(c); ++p) {
            int ra, rb;
            CHK(dist_owned_rows(c, p, &ra, &rb));
            held.push_back({ra, rb});
        }
    } else {
        held.push_back({0, c->N + 1});
    }
    for (long k = 0; k < npts; ++k) {
        if (pi[k] < 0 || pi[k] > c->N || pj[k] < 0 || pj[k] > c->N)
            return fail(MGX_E_ARG, std::string(who) + ": point k = " + std::to_string(k) +
                                       " lies outside the grid (0 <= pi, pj <= N)");
        bool ok = false;
        for (const auto &r : held) ok = ok || (pi[k] >= r.first && pi[k] < r.second);
        if (!ok)
            return fail(MGX_E_ARG, std::string(who) + ": point k = " + std::to_string(k) +
                                       " lies in a row this rank does not own");
    }
    HIPCHK(hipSetDevice(c->device));
    long *di, *dj;
    double *dv;
    CHK(dense_staging(c, npts, &di, &dj, &dv));
    HIPCHK(hipMemcpyAsync(di, pi, sizeof(long) * (size_t)npts, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dj, pj, sizeof(long) * (size_t)npts, hipMemcpyHostToDevice, c->stream));
    CHK(dense_points_launch(c, order + 1, w, npts, di, dj, dv));
    HIPCHK(hipMemcpyAsync(out, dv, sizeof(double) * (size_t)npts, hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MGX_OK;
}
int mgx_dense_points_device(mgx_ctx *c, int order, double tau, long npts, const long *pi,
                            const long *pj, double *out) {
    const char *who = "mgx_dense_points_device";
    double w[3];
    CHK(dense_check(c, order, tau, who, w));
    if (npts < 0) return fail(MGX_E_ARG, std::string(who) + ": npts must be >= 0");
    if (npts > 0 && (!pi || !pj || !out))
        return fail(MGX_E_ARG, std::string(who) + ": null argument");
    mgxdense::timer_reset();
    if (npts == 0) return MGX_OK;
    HIPCHK(hipSetDevice(c->device));
    return dense_points_launch(c, order + 1, w, npts, pi, pj, out);
}
int mgx_array_dense(double *out, const double *u, const double *h, const double *h2, long n,
                    double w0, double w1, double w2, int levels) {
    if (levels < 1 || levels > 3)
        return fail(MGX_E_ARG, "mgx_array_dense: levels must be 1, 2 or 3");
    if (!out || !u || (levels >= 2 && !h) || (levels >= 3 && !h2))
        return fail(MGX_E_ARG, "mgx_array_dense: null argument");
    if (n < 1) return fail(MGX_E_ARG, "mgx_array_dense: n must be >= 1");
    mgxdense::timer_reset();
    mgxdense::PassTimer T;
    T.begin(nullptr);
    mgxdense::launch_raw(out, u, h, h2, n, w0, w1, w2, levels, nullptr);
    T.end(nullptr);
    CHK(check_launch("mgx_array_dense"));
    HIPCHK(hipStreamSynchronize(nullptr));
    T.commit(8.0 * (levels + 1) * (double)(n + 1) * (double)(n + 1));
    return MGX_OK;
}

}  // extern "C"

// ---- time-dependent Dirichlet data (include/mgx.h, csrc/boundary.hip)
// Everything formed with the old ring goes -- what mgx_set_source drops, and a
// deferred coarsest solve -- after a packed u_pre has been expanded, so that
// the current buffer holds whole rows for the scatter.  Captured sub-cycles
// stay: they hold no finest-level value.
int mgxi::boundary_prepare_ctx(mgx_ctx *c) {
    CHK(materialize(c, 0));
    CHK(op_expand(c));
    drop_source_state(c);
    c->cf_level = -1;
    c->cf_reps = 0;
    return MGX_OK;
}
// Only the current buffer is written: every pass that writes a finest-level u
// buffer writes its ring from its input (kernels.h launch_smooth: every point
// of uout, boundary included; xsmooth.hip: the guarded kernel owns the whole
// boundary and takes it from its input), never from what the output held.
int mgxi::boundary_scatter_ctx(mgx_ctx *c, const double *g) {
    Level &L = c->lv[0];
    mgxbc::launch_scatter(L.U(), L.pitch, L.n, 0, L.n, g, c->stream);
    return check_launch("mgx_set_boundary: ring scatter");
}

// MGX_BC_NOW with a device ring on any context; c->bc_timer spans the scatter
// launches (committed by the caller once the stream has passed them)
static int boundary_now(mgx_ctx *c, const double *g) {
    if (c->dist) return dist_boundary_now(c, g);
    CHK(boundary_prepare_ctx(c));
    c->bc_timer.begin(c->stream);
    const int rc = boundary_scatter_ctx(c, g);
    c->bc_timer.end(c->stream);
    return rc;
}

// the context's two rings (ctx.h bc_buf), allocated by the first call that needs one
static int bc_buffers(mgx_ctx *c, const char *who) {
    if (c->bc_buf) return MGX_OK;
    const hipError_t e = hipMalloc(&c->bc_buf, sizeof(double) * 2 * (size_t)mgxbc::ring_size(c->N));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        c->bc_buf = nullptr;
        return fail(MGX_E_HIP, std::string(who) + ": no room for the context's copy of the ring: " +
                                   hipGetErrorString(e));
    }
    return MGX_OK;
}

static int set_boundary_impl(mgx_ctx *c, const double *g, int when, hipMemcpyKind kind,
                             const char *who) {
    if (!c) return fail(MGX_E_ARG, std::string(who) + ": null ctx");
    if (when != MGX_BC_NOW && when != MGX_BC_NEXT_STEP)
        return fail(MGX_E_ARG, std::string(who) + ": when must be MGX_BC_NOW or MGX_BC_NEXT_STEP");
    if (!g) {
        if (when == MGX_BC_NOW) return fail(MGX_E_ARG, std::string(who) + ": null ring");
        c->bc_pending = false;   // cancels a pending ring
        return MGX_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    const size_t bytes = sizeof(double) * (size_t)mgxbc::ring_size(c->N);
    if (when == MGX_BC_NEXT_STEP) {
        CHK(bc_buffers(c, who));
        // a prepared next step took its initial norm and its pre-smoothing with
        // the old ring
        if (c->step_spec) drop_spec(c);
        c->bc_pending = false;
        HIPCHK(hipMemcpyAsync(c->bc_buf, g, bytes, kind, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));   // the caller's buffer is free on return
        c->bc_pending = true;
        return MGX_OK;
    }
    const double *dg = g;
    if (kind == hipMemcpyHostToDevice) {
        CHK(bc_buffers(c, who));
        double *stage = c->bc_buf + mgxbc::ring_size(c->N);
        HIPCHK(hipMemcpyAsync(stage, g, bytes, kind, c->stream));
        dg = stage;
    }
    CHK(boundary_now(c, dg));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->bc_timer.commit();
    return MGX_OK;
}

static int get_boundary_impl(mgx_ctx *c, double *g, hipMemcpyKind kind, const char *who) {
    if (!c) return fail(MGX_E_ARG, std::string(who) + ": null ctx");
    if (!g) return fail(MGX_E_ARG, std::string(who) + ": null ring");
    const bool host = kind == hipMemcpyDeviceToHost;
    double *dg = g;
    if (c->dist) {
        CHK(dist_boundary_gather(c, nullptr, who));   // (the checks alone)
        HIPCHK(hipSetDevice(c->device));
        if (host) {
            CHK(bc_buffers(c, who));
            dg = c->bc_buf + mgxbc::ring_size(c->N);
        }
        CHK(dist_boundary_gather(c, dg, who));
    } else {
        HIPCHK(hipSetDevice(c->device));
        if (host) {
            CHK(bc_buffers(c, who));
            dg = c->bc_buf + mgxbc::ring_size(c->N);
        }
        CHK(materialize(c, 0));
        CHK(op_expand(c));   // as mgx_download
        Level &L = c->lv[0];
        mgxbc::launch_gather(L.U(), L.pitch, L.n, 0, 0, L.n, dg, c->stream);
        CHK(check_launch(who));
    }
    if (host)
        HIPCHK(hipMemcpyAsync(g, dg, sizeof(double) * (size_t)mgxbc::ring_size(c->N), kind,
                              c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MGX_OK;
}

extern "C" {

int mgx_set_boundary(mgx_ctx *c, const double *g, int when) {
    return set_boundary_impl(c, g, when, hipMemcpyHostToDevice, "mgx_set_boundary");
}
int mgx_set_boundary_device(mgx_ctx *c, const double *g, int when) {
    return set_boundary_impl(c, g, when, hipMemcpyDeviceToDevice, "mgx_set_boundary_device");
}
int mgx_get_boundary(mgx_ctx *c, double *g) {
    return get_boundary_impl(c, g, hipMemcpyDeviceToHost, "mgx_get_boundary");
}
int mgx_get_boundary_device(mgx_ctx *c, double *g) {
    return get_boundary_impl(c, g, hipMemcpyDeviceToDevice, "mgx_get_boundary_device");
}
int mgx_boundary_info(mgx_ctx *c, int *pending) {
    if (!c) return fail(MGX_E_ARG, "mgx_boundary_info: null ctx");
    if (!pending) return fail(MGX_E_ARG, "mgx_boundary_info: null argument");
    *pending = c->bc_pending ? 1 : 0;
    return MGX_OK;
}
int mgx_write_boundary(double *u, long n, const double *g) {
    if (!u || !g) return fail(MGX_E_ARG, "mgx_write_boundary: null pointer");
    if (n < 1) return fail(MGX_E_ARG, "mgx_write_boundary: n must be >= 1");
    mgxbc::launch_scatter(u, n + 1, n, 0, n, g, nullptr);
    return check_launch("mgx_write_boundary");
}

}  // extern "C"

// ---- per-step dt and theta (include/mgx.h, csrc/tstep.hip)
void mgxi::step_coefs(const mgx_ctx *c, double h, mgx::Coef *coef, mgx::Coef *coef_rhs) {
    *coef = mgx::make_coef(c->k_solve(), c->nu, h, c->opt.fp_mode == MGX_FP_FMA);
    // (k_bdf set: a BDF2 step forms its own right-hand side; the theta-scheme's
    // coefficients come back, k_bdf = 0, before anything reads coef_rhs)
    *coef_rhs = c->two_op() || c->k_bdf != 0 ? mgx::make_coef(c->kB(), c->nu, h) : *coef;
}
// Everything formed with the old coefficients goes: what mgx_set_boundary
// drops, and the captured sub-cycles -- unlike a ring, the coefficients are
// kernel arguments of every node of a graph.
int mgxi::retime_ctx(mgx_ctx *c, double dt, double theta, double k_bdf) {
    drop_source_state(c);
    c->cf_level = -1;
    c->cf_reps = 0;
    // (a replay may still be running: free_ctx drains the stream first too)
    if (!c->graphs.empty()) HIPCHK(hipStreamSynchronize(c->stream));
    free_graphs(c);
    c->dt = dt;
    c->theta = theta;
    c->k_bdf = k_bdf;
    for (Level &L : c->lv) step_coefs(c, L.coef.h, &L.coef, &L.coef_rhs);
    return MGX_OK;
}

extern "C" {

int mgx_set_time_step(mgx_ctx *c, double dt, double theta) {
    if (!c) return fail(MGX_E_ARG, "mgx_set_time_step: null ctx");
    if (!std::isfinite(dt) || !(dt > 0))
        return fail(MGX_E_ARG, "mgx_set_time_step: dt must be finite and > 0");
    if (!std::isfinite(theta) || !(theta > 0) || !(theta <= 1))
        return fail(MGX_E_ARG, "mgx_set_time_step: theta must satisfy 0 < theta <= 1");
    HIPCHK(hipSetDevice(c->device));
    if (c->dist) return dist_set_time_step(c, dt, theta);
    // a packed u_pre is expanded with the operator that packed it
    CHK(materialize(c, 0));
    CHK(op_expand(c));
    return retime_ctx(c, dt, theta);
}
int mgx_time_step_info(mgx_ctx *c, double *dt, double *theta) {
    if (!c) return fail(MGX_E_ARG, "mgx_time_step_info: null ctx");
    if (dt) *dt = c->dt;
    if (theta) *theta = c->theta;
    return MGX_OK;
}

static int no_dist(mgx_ctx *c, const char *what) {
    return fail(MGX_E_ARG, std::string(what) + ": per-level ops are not available on a "
                                               "partitioned context (use vcycle/mg_outer/step)");
}
// The solve side of every level with k = k_bdf (a BDF2 step's kA), or the
// theta-scheme's again (0): mgx_set_time_step with the context's own dt and
// theta -- the same drops, a packed u_pre expanded first with the operator
// that packed it.
static int set_solve_k(mgx_ctx *c, double k_bdf) {
    HIPCHK(hipSetDevice(c->device));
    if (c->dist) return dist_set_time_step(c, c->dt, c->theta, k_bdf);
    CHK(materialize(c, 0));
    CHK(op_expand(c));
    return retime_ctx(c, c->dt, c->theta, k_bdf);
}
int mgx_rhs(mgx_ctx *c) {
    if (!c) return fail(MGX_E_ARG, "null ctx");
    if (c->k_bdf != 0) CHK(set_solve_k(c, 0.0));   // after mgx_step_bdf2
    if (c->dist) return dist_rhs(c);
    return op_rhs(c);
}
int mgx_gs(mgx_ctx *c, int level, int sweeps) {
    if (!c || level < 0 || level >= c->L || sweeps < 0) return fail(MGX_E_ARG, "mgx_gs: bad args");
    if (c->dist) return no_dist(c, "mgx_gs");
    drop_spec(c);
    return op_gs(c, level, sweeps);
}
int mgx_residual_norm(mgx_ctx *c, int level, double *norm) {
    if (!c || level < 0 || level >= c->L || !norm) return fail(MGX_E_ARG, "mgx_residual_norm: bad args");
    if (c->dist) {
        if (level != 0) return no_dist(c, "mgx_residual_norm");
        return dist_residual_norm(c, norm);
    }
    return op_residual_norm(c, level, norm);
}
int mgx_restrict(mgx_ctx *c, int level) {
    if (!c || level < 0 || level >= c->L - 1) return fail(MGX_E_ARG, "mgx_restrict: bad level");
    if (c->dist) return no_dist(c, "mgx_restrict");
    drop_spec(c);
    return op_restrict(c, level);
}
int mgx_prolong_add(mgx_ctx *c, int level) {
    if (!c || level < 0 || level >= c->L - 1) return fail(MGX_E_ARG, "mgx_prolong_add: bad level");
    if (c->dist) return no_dist(c, "mgx_prolong_add");
    drop_spec(c);
    return op_prolong_add(c, level);
}
// A pending next-step state (mgx_step) is only valid for the next mgx_step.
static void drop_step_spec(mgx_ctx *c) {
    if (c->step_spec) drop_spec(c);
}
int mgx_vcycle(mgx_ctx *c) {
    if (!c) return fail(MGX_E_ARG, "null ctx");
    drop_step_spec(c);
    if (c->dist) return dist_vcycle(c, nullptr);
    return op_vcycle(c, 0);
}
int mgx_mg_outer(mgx_ctx *c, double tol, int *cycles, double *res0, double *res) {
    if (!c) return fail(MGX_E_ARG, "null ctx");
    drop_step_spec(c);
    return op_mg_outer(c, tol, cycles, res0, res);
}
// tuning key "step_cross": 1 (default) = mgx_step's last cycle also forms the
// next step's rhs, initial norm and first pre-smoothing (cross pass in step
// mode), consumed by the next mgx_step; 0 = each step starts with its own
// rhs + norm pass
long g_step_cross = 1;

// Step mode needs a second finest-level rhs (the next step's, written by the
// cross pass).  It is allocated on first use, outside any pass; when HBM is
// too short for it (N=65536 on one GPU: the towers take ~265 of 288 GB) the
// context runs the plain schedule instead -- the same results, one pass more
// per step.
static bool step_rhs_alt(mgx_ctx *c) {
    Level &L = c->lv[0];
    if (L.rhs_alt) return true;
    if (c->no_rhs_alt || !cross_ok(c) || !mgx::xstep_supported(L.n)) return false;
    const size_t bytes = sizeof(double) * (size_t)(L.n + 1) * (size_t)L.pitch;
    if (hipMalloc(&L.rhs_alt, bytes) != hipSuccess) {
        (void)hipGetLastError();   // out of memory is not an error here
        L.rhs_alt = nullptr;
        c->no_rhs_alt = true;
        return false;
    }
    // zero boundary: compute_rhs writes the interior only
    if (hipMemsetAsync(L.rhs_alt, 0, bytes, c->stream) != hipSuccess) {
        (void)hipFree(L.rhs_alt);
        L.rhs_alt = nullptr;
        c->no_rhs_alt = true;
        return false;
    }
    return true;
}

static int step_impl(mgx_ctx *c, double tol, int *cycles, bool prepare_next,
                     double *res0_out = nullptr, double *res_out = nullptr) {
    // compute_rhs and mg_outer's initial norm in one pass (timestepper,
    // multigrid.cpp:168-170), with the first pre-smoothing where it fuses --
    // or already done by the previous step's last cross pass
    double res0 = 0;
    if (c->k_bdf != 0) CHK(set_solve_k(c, 0.0));   // after mgx_step_bdf2
    if (c->hist_on) {   // mgx_set_history: h = u^n, before a pending ring is written
        if (c->hist2_on) {   // depth 2: the copy goes into the older buffer
            hist_swap(c);
            c->hist2_valid = c->hist_valid;
            c->hist2_dt = c->hist_dt;
            c->hist_valid = false;   // (until the copy below is issued)
        }
        c->hist_rolled = false;
        CHK(c->dist ? dist_snapshot(c) : hist_snapshot_ctx(c));
        c->hist_dt = c->dt;
        c->hist_valid = true;
    }
    if (c->bc_pending) {
        // a pending ring (mgx_set_boundary, MGX_BC_NEXT_STEP): the rhs with the
        // old ring, the new ring, then mg_outer with its own initial norm --
        // mgx_rhs; mgx_set_boundary(MGX_BC_NOW); mgx_mg_outer, launch for
        // launch.  No fusion across the ring write, and no next step prepared:
        // its ring will be set again.
        CHK(c->dist ? dist_rhs(c) : op_rhs(c));
        c->bc_pending = false;
        CHK(boundary_now(c, c->bc_buf));
        drop_step_spec(c);
        const int rc = op_mg_outer(c, tol, cycles, res0_out, res_out);
        c->bc_timer.commit();   // (mg_outer's norm reads have passed the scatter)
        return rc;
    }
    if (c->step_spec && !c->dist) {
        Level &L = c->lv[0];
        std::swap(L.rhs, L.rhs_alt);
        res0 = c->step_res0;
        c->step_spec = false;   // lv[0].spec and lv[1]'s rhs stay: the first cycle's
    } else if (c->dist) {
        CHK(dist_rhs_norm(c, &res0));
    } else if (c->two_op()) {
        CHK(op_rhs_norm2(c, &res0));
    } else if (!c->has_source() && step_fusable(c)) {
        CHK(op_rhs_norm_pre(c, &res0));
    } else {
        CHK(op_rhs_norm(c, &res0));
    }
    // (a source: both fused forms make the rhs inside kernels that know none --
    // k_wsmooth's kModeRhsNorm above, the cross pass's step mode here; theta !=
    // 1/2: both form the rhs and smooth with one Coef; a history: the next
    // step may be a BDF2 one)
    c->step_next = prepare_next && g_step_cross != 0 && !c->dist && !c->has_source() &&
                   !c->two_op() && !c->hist_on && step_rhs_alt(c);
    const int rc = op_mg_outer(c, tol, cycles, res0_out, res_out, &res0);
    c->step_next = false;
    return rc;
}
int mgx_step(mgx_ctx *c, double tol, int *cycles) {
    if (!c) return fail(MGX_E_ARG, "null ctx");
    return step_impl(c, tol, cycles, true);
}
int mgx_step_ex(mgx_ctx *c, double tol, int *cycles, double *res0, double *res) {
    if (!c) return fail(MGX_E_ARG, "mgx_step_ex: null ctx");
    return step_impl(c, tol, cycles, true, res0, res);
}

// ---- variable-step BDF2 on a device-resident history (include/mgx.h, csrc/bdf.hip)
int mgx_bdf2_coefficients(double dt, double dt_prev, double *g, double *b0, double *b1,
                          double *kA) {
    if (!std::isfinite(dt) || !(dt > 0))
        return fail(MGX_E_ARG, "mgx_bdf2_coefficients: dt must be finite and > 0");
    if (!std::isfinite(dt_prev) || !(dt_prev > 0))
        return fail(MGX_E_ARG, "mgx_bdf2_coefficients: dt_prev must be finite and > 0");
    const mgxbdf::Coefs k = mgxbdf::coefficients(dt, dt_prev);
    if (g) *g = k.g;
    if (b0) *b0 = k.b0;
    if (b1) *b1 = k.b1;
    if (kA) *kA = k.kA;
    return MGX_OK;
}
int mgx_set_history(mgx_ctx *c, int on) {
    if (!c) return fail(MGX_E_ARG, "mgx_set_history: null ctx");
    if (on != 0 && on != 1) return fail(MGX_E_ARG, "mgx_set_history: on must be 0 or 1");
    if (on && c->hist_on) return MGX_OK;
    if (!on && !c->hist_on) return MGX_OK;
    HIPCHK(hipSetDevice(c->device));
    if (on) {
        // a prepared next step belongs to a schedule that a history turns off
        if (c->dist)
            CHK(dist_set_history(c, 1, "mgx_set_history"));
        else
            CHK(hist_alloc_ctx(c, "mgx_set_history"));
        drop_step_spec(c);
        c->hist_on = true;
        c->hist_valid = false;
        c->hist_dt = 0;
        return MGX_OK;
    }
    if (c->dist)
        CHK(dist_set_history(c, 0, "mgx_set_history"));
    else
        hist_free_ctx(c);
    c->hist_on = false;
    c->hist2_on = false;
    c->hist_invalidate();
    c->hist_dt = 0;
    c->hist2_dt = 0;
    return MGX_OK;
}
int mgx_set_history_depth(mgx_ctx *c, int depth) {
    if (!c) return fail(MGX_E_ARG, "mgx_set_history_depth: null ctx");
    if (depth < 0 || depth > 2)
        return fail(MGX_E_ARG, "mgx_set_history_depth: depth must be 0, 1 or 2");
    const int have = c->hist_on ? (c->hist2_on ? 2 : 1) : 0;
    if (depth == have) return MGX_OK;
    if (depth == 0) return mgx_set_history(c, 0);
    if (have == 0) CHK(mgx_set_history(c, 1));
    if (depth == 1) {   // 2 -> 1: the older array goes
        HIPCHK(hipSetDevice(c->device));
        if (c->dist)
            CHK(dist_set_history2(c, 0, false, "mgx_set_history_depth"));
        else
            hist2_free_ctx(c);
        c->hist2_on = c->hist2_valid = false;   // (hist_rolled stays until the next step)
        c->hist2_dt = 0;
        return MGX_OK;
    }
    // -> 2, all parts or none; a failure leaves the depth the context had
    HIPCHK(hipSetDevice(c->device));
    const bool zero_hist = !c->hist_valid;
    int rc;
    if (c->dist) {
        rc = dist_set_history2(c, 1, zero_hist, "mgx_set_history_depth");
    } else {
        rc = hist2_alloc_ctx(c, zero_hist, "mgx_set_history_depth");
        if (rc != MGX_OK) hist2_free_ctx(c);
    }
    if (rc != MGX_OK) {
        if (have == 0) {   // (mgx_set_history keeps the message of the failure intact)
            const std::string msg = mgx_last_error();
            (void)mgx_set_history(c, 0);
            return fail(rc, msg);
        }
        return rc;
    }
    c->hist2_on = true;
    c->hist2_valid = false;
    c->hist2_dt = 0;
    return MGX_OK;
}
int mgx_history_depth(mgx_ctx *c, int *depth, int *valid2, double *dt_prev2) {
    if (!c) return fail(MGX_E_ARG, "mgx_history_depth: null ctx");
    if (depth) *depth = c->hist_on ? (c->hist2_on ? 2 : 1) : 0;
    if (valid2) *valid2 = c->hist2_valid ? 1 : 0;
    if (dt_prev2) *dt_prev2 = c->hist2_dt;
    return MGX_OK;
}
int mgx_history_info(mgx_ctx *c, int *on, int *valid, double *dt_prev, double *k_solve) {
    if (!c) return fail(MGX_E_ARG, "mgx_history_info: null ctx");
    if (on) *on = c->hist_on ? 1 : 0;
    if (valid) *valid = c->hist_valid ? 1 : 0;
    if (dt_prev) *dt_prev = c->hist_dt;
    if (k_solve) *k_solve = c->k_solve();
    return MGX_OK;
}
// A BDF2 step with a predicted start (mgx_set_predictor; csrc/predict.h) on a
// single-GPU context with no ring pending.  The pass reads u^n, u^(n-1) (and
// u^(n-2)) at stencil neighbours and writes the guess into level 0's free
// buffer, so no array it reads may be written by it: the history moves on by an
// exchange of pointers.  Every array in the exchange is a finest-level array of
// pitch * (n + 1) doubles from its own hipMalloc (create_ctx, hist_alloc_ctx,
// hist2_alloc_ctx) whose padding columns are zeros -- each has been zeroed or a
// whole copy of u -- and nothing holds a level-0 u pointer across calls (the
// captured sub-cycles start at level >= 1; every pass takes L.U(), hist and
// hist2 at call time).
static int step_bdf2_predicted(mgx_ctx *c, const mgxbdf::Coefs &K, double cf, double tol,
                               int *cycles, double *res0_out, double *res_out) {
    const int e = c->pred_order == 2 && c->hist2_on && c->hist2_valid ? 2 : 1;
    double w[3];
    if (mgxdense::weights(e, c->dt, c->hist_dt, c->hist2_dt, w) != 0)
        return fail(MGX_E_INTERNAL, "mgx_step_bdf2: the predictor's weights");
    double r0 = 0, rp = 0;
    CHK(op_predict_bdf(c, K.b0, K.b1, cf, e, w, &r0, &rp));
    Level &L = c->lv[0];
    if (!L.u[L.cur] || !L.u[L.nxt()] || !c->hist || (c->hist2_on && !c->hist2))
        return fail(MGX_E_INTERNAL, "mgx_step_bdf2: a finest-level array is missing");
    // the buffer of u^n becomes hist, the old hist becomes hist2 (depth 2), and
    // the oldest history array takes u^n's place among level 0's buffers
    double *un = L.u[L.cur], *spare = nullptr;
    if (c->hist2_on) {
        spare = c->hist2;
        c->hist2 = c->hist;
        c->hist2_valid = true;
        c->hist2_dt = c->hist_dt;
    } else {
        spare = c->hist;
    }
    c->hist = un;
    L.u[L.cur] = spare;
    L.packed[L.cur] = false;
    c->hist_rolled = false;
    c->hist_dt = c->dt;
    const bool adopted = rp < r0;   // (false where rp is NaN)
    c->pred_last = e;
    c->pred_adopted = adopted;
    c->pred_res = rp;
    if (adopted) {
        L.cur = L.nxt();   // the guess
    } else {
        // refused: u^n is both u and h -- one copy, as a theta-step's snapshot
        const size_t bytes = sizeof(double) * (size_t)(L.n + 1) * (size_t)L.pitch;
        HIPCHK(hipMemcpyAsync(L.u[L.cur], c->hist, bytes, hipMemcpyDeviceToDevice, c->stream));
    }
    L.zero = false;
    return op_mg_outer(c, tol, cycles, res0_out, res_out, &r0, adopted ? &rp : nullptr);
}
int mgx_set_predictor(mgx_ctx *c, int order) {
    if (!c) return fail(MGX_E_ARG, "mgx_set_predictor: null ctx");
    if (order < 0 || order > 2)
        return fail(MGX_E_ARG, "mgx_set_predictor: order must be 0, 1 or 2");
    if (order > 0 && c->dist)
        return fail(MGX_E_ARG, "mgx_set_predictor: a partitioned context takes order 0 only (the "
                               "guess would need a ghost-row exchange)");
    c->pred_order = order;
    return MGX_OK;
}
int mgx_predictor_info(mgx_ctx *c, int *order, int *last_order, int *adopted, double *res_pred) {
    if (!c) return fail(MGX_E_ARG, "mgx_predictor_info: null ctx");
    if (order) *order = c->pred_order;
    if (last_order) *last_order = c->pred_last;
    if (adopted) *adopted = c->pred_adopted ? 1 : 0;
    if (res_pred) *res_pred = c->pred_last ? c->pred_res : 0.0;
    return MGX_OK;
}
int mgx_step_bdf2(mgx_ctx *c, double tol, int *cycles, double *res0_out, double *res_out) {
    if (!c) return fail(MGX_E_ARG, "mgx_step_bdf2: null ctx");
    if (!c->hist_on)
        return fail(MGX_E_ARG, "mgx_step_bdf2: the context has no history (mgx_set_history)");
    if (!c->hist_valid)
        return fail(MGX_E_ARG, "mgx_step_bdf2: the history is not valid: it holds no u^(n-1) "
                               "(a theta-step, mgx_step, starts it)");
    const mgxbdf::Coefs K = mgxbdf::coefficients(c->dt, c->hist_dt);
    const double cf = (K.g * c->dt) * c->src_scale;
    if (K.kA != c->k_solve()) CHK(set_solve_k(c, K.kA));
    HIPCHK(hipSetDevice(c->device));
    drop_step_spec(c);
    c->pred_last = 0;
    c->pred_adopted = false;
    c->pred_res = 0;
    // (a step that takes a pending ring runs unpredicted, launch for launch)
    if (c->pred_order > 0 && !c->bc_pending && !c->dist)
        return step_bdf2_predicted(c, K, cf, tol, cycles, res0_out, res_out);
    // rhs, h <- u^n and mg_outer's initial norm in one pass
    double res0 = 0;
    if (c->hist2_on) {
        // depth 2: u^(n-1) is read where it lies and u^n stored into the older
        // buffer -- no byte more than at depth 1
        hist_swap(c);
        c->hist2_valid = true;
        c->hist2_dt = c->hist_dt;
    }
    c->hist_rolled = false;
    if (c->dist)
        CHK(dist_rhs_norm_bdf(c, K.b0, K.b1, cf, &res0));
    else
        CHK(op_rhs_norm_bdf(c, K.b0, K.b1, cf, &res0));
    c->hist_dt = c->dt;
    if (c->bc_pending) {
        // a pending ring: written after the pass, and mg_outer takes its own
        // initial norm, as step_impl orders it
        c->bc_pending = false;
        CHK(boundary_now(c, c->bc_buf));
        const int rc = op_mg_outer(c, tol, cycles, res0_out, res_out);
        c->bc_timer.commit();
        return rc;
    }
    return op_mg_outer(c, tol, cycles, res0_out, res_out, &res0);
}
int mgx_rollback(mgx_ctx *c) {
    if (!c) return fail(MGX_E_ARG, "mgx_rollback: null ctx");
    if (!c->hist_on || !c->hist_valid)
        return fail(MGX_E_ARG, "mgx_rollback: the context has no valid history (mgx_set_history, "
                               "then a step)");
    if (c->hist_rolled)
        return fail(MGX_E_ARG, "mgx_rollback: the step has been rolled back already: the history "
                               "holds u^(n-1) for the next mgx_step_bdf2, not the u to go back to");
    HIPCHK(hipSetDevice(c->device));
    if (c->dist)
        CHK(dist_rollback(c));
    else
        CHK(hist_restore_ctx(c));
    if (c->hist2_on && c->hist2_valid) {
        // depth 2: u^(n-1) and its dt become the history again, so the retry
        // may be a BDF2 step at any dt
        hist_swap(c);
        c->hist_dt = c->hist2_dt;
        c->hist2_valid = false;
        c->hist_rolled = true;
    } else {
        c->hist_valid = false;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return MGX_OK;
}
int mgx_compute_rhs_bdf2(double *rhs, const double *u, const double *h, long n, double b0,
                         double b1, const double *f, double c) {
    if (!rhs || !u || !h) return fail(MGX_E_ARG, "mgx_compute_rhs_bdf2: null pointer");
    if (n < 2) return fail(MGX_E_ARG, "mgx_compute_rhs_bdf2: n must be >= 2");
    mgxbdf::launch_raw_rhs_bdf(rhs, u, h, n, b0, b1, f, c, nullptr);
    return check_launch("mgx_compute_rhs_bdf2");
}

int mgx_run_cycles(mgx_ctx *c, int cycles, double *res) {
    if (!c || cycles < 0) return fail(MGX_E_ARG, "mgx_run_cycles: bad args");
    drop_step_spec(c);
    double r = 0;
    c->fixed_cycles = true;
    int rc = MGX_OK;
    for (int k = 0; k < cycles && rc == MGX_OK; ++k)
        rc = cycle_norm(c, &r, /*store_post=*/k == cycles - 1);
    c->fixed_cycles = false;
    CHK(rc);
    if (res) *res = r;
    return MGX_OK;
}

int mgx_level_n(mgx_ctx *c, int level, long *n) {
    if (!c || !n || level < 0 || level >= c->L) return fail(MGX_E_ARG, "mgx_level_n: bad args");
    *n = c->N >> level;
    return MGX_OK;
}
int mgx_coarse_iterations(mgx_ctx *c, long *iters) {
    if (!c || !iters) return fail(MGX_E_ARG, "bad args");
    if (c->dist) c = dist_sub(c, 0);   // every rank runs the same replicated coarse solve
    HIPCHK(hipMemcpyAsync(c->hscal + 2, c->dscal + 2, 2 * sizeof(double), hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *iters = (long)(c->hscal[2] + c->hscal[4]);
    return MGX_OK;
}
int mgx_stream(mgx_ctx *c, void **stream) {
    if (!c || !stream) return fail(MGX_E_ARG, "bad args");
    *stream = (void *)c->stream;
    return MGX_OK;
}
int mgx_synchronize(mgx_ctx *c) {
    if (!c) return fail(MGX_E_ARG, "null ctx");
    // (partitioned: the side stream's exchanges too -- no RCCL operation of
    // the context is in flight when this returns)
    if (c->dist) CHK(dist_settle(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MGX_OK;
}

int mgx_profile_enable(mgx_ctx *c, int on) {
    if (!c) return fail(MGX_E_ARG, "null ctx");
    CHK(prof_flush(c));
    if (on < 0 || on > 2) return fail(MGX_E_ARG, "mgx_profile_enable: on must be 0, 1 or 2");
    c->prof = on;
    // the replicated levels of a partitioned context are not the finest,
    // unless everything is replicated (first replicated level 0)
    const int sub_on = on == 1 ? 1 : (on == 2 && dist_la(c) == 0 ? 2 : 0);
    for (int i = 0; i < dist_nsub(c); ++i) CHK(mgx_profile_enable(dist_sub(c, i), sub_on));
    return MGX_OK;
}
int mgx_profile_reset(mgx_ctx *c) {
    if (!c) return fail(MGX_E_ARG, "null ctx");
    CHK(prof_flush(c));
    memset(c->sum_ms, 0, sizeof(c->sum_ms));
    memset(c->sum_bytes, 0, sizeof(c->sum_bytes));
    memset(c->sum_cbytes, 0, sizeof(c->sum_cbytes));
    memset(c->count, 0, sizeof(c->count));
    for (int i = 0; i < dist_nsub(c); ++i) CHK(mgx_profile_reset(dist_sub(c, i)));
    return MGX_OK;
}
// Partitioned contexts: the replicated levels' launches (sub-contexts, level
// numbers shifted by the first replicated level) are included.
int mgx_profile_get_ex(mgx_ctx *c, int kind, int level, long *launches, double *ms,
                       double *bytes, double *cbytes) {
    if (!c || kind < 0 || kind >= MGX_K_COUNT || level >= 64)
        return fail(MGX_E_ARG, "mgx_profile_get: bad args");
    CHK(prof_flush(c));
    long n = 0;
    double t = 0, b = 0, cb = 0;
    for (int l = 0; l < 64; ++l) {
        if (level >= 0 && l != level) continue;
        n += c->count[kind][l];
        t += c->sum_ms[kind][l];
        b += c->sum_bytes[kind][l];
        cb += c->sum_cbytes[kind][l];
    }
    const int la = dist_la(c);
    for (int i = 0; i < dist_nsub(c); ++i) {
        if (level >= 0 && level < la) break;
        long sn = 0;
        double st = 0, sb = 0, scb = 0;
        CHK(mgx_profile_get_ex(dist_sub(c, i), kind, level < 0 ? -1 : level - la, &sn, &st, &sb,
                               &scb));
        n += sn;
        t += st;
        b += sb;
        cb += scb;
    }
    if (launches) *launches = n;
    if (ms) *ms = t;
    if (bytes) *bytes = b;
    if (cbytes) *cbytes = cb;
    return MGX_OK;
}
int mgx_profile_get(mgx_ctx *c, int kind, int level, long *launches, double *ms, double *bytes) {
    return mgx_profile_get_ex(c, kind, level, launches, ms, bytes, nullptr);
}

// ---- timestepper (multigrid.cpp:124-186)
int mgx_timestepper_ex(double *uT, const double *u0, const double *v1, const double *v2,
                       double nu, int maxlvl, long n, double dt, double T, double dx, double tol,
                       const mgx_options *opt, int *cycles_per_step) {
    (void)dx;   // the context derives dx = 1/n (multigrid.cpp:194)
    if (!uT || !u0 || !v1 || !v2) return fail(MGX_E_ARG, "mgx_timestepper: null array");
    mgx_ctx *c = nullptr;
    CHK(mgx_create(&c, n, maxlvl, dt, nu, opt));
    int rc = mgx_upload(c, u0, v1, v2);
    const int steps = (int)(T / dt);   // multigrid.cpp:165
    for (int it = 0; rc == MGX_OK && it < steps; ++it) {
        int cyc = 0;
        rc = step_impl(c, tol, &cyc, /*prepare_next=*/it + 1 < steps);
        if (rc == MGX_E_NOCONV) {
            // multigrid.cpp:117-119 only warns; keep stepping
            printf("multigrid did not converge in %d cycles\n", c->opt.max_cycle);
            rc = MGX_OK;
        }
        if (cycles_per_step) cycles_per_step[it] = cyc;
    }
    if (rc == MGX_OK) rc = mgx_download(c, uT);
    std::string keep = g_err;
    mgx_destroy(c);
    g_err = keep;
    return rc;
}

int mgx_timestepper(double *uT, const double *u0, const double *v1, const double *v2, double nu,
                    int maxlvl, long n, double dt, double T, double dx, double tol, int shape) {
    mgx_options o;
    mgx_default_options(&o);
    o.shape = shape;
    return mgx_timestepper_ex(uT, u0, v1, v2, nu, maxlvl, n, dt, T, dx, tol, &o, nullptr);
}

}  // extern "C"

// ---- reference problem setup (multigrid.cpp:206-233), host, glibc libm
#include <thread>
// Rows [r0, r1) of the reference problem (multigrid.cpp:206-233) into arrays
// holding just those rows; bitwise the rows of the full initialisation.
static int init_rows(double *u0, double *v1, double *v2, long N, long r0, long r1,
                     int nthreads) {
    const double PI = 3.1415926535897932;   // multigrid.cpp:14
    const double dx = 1.0 / N;
    const double x0 = 0.2, y0 = 0.4, sigma = 100.0, kx = 1.0 * PI, ky = 1.0 * PI;
    const long w = N + 1;
    int nt = nthreads > 0 ? nthreads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > r1 - r0) nt = (int)std::max<long>(1, r1 - r0);
    auto rows = [&](long a, long b) {
        for (long i = a; i < b; ++i) {
            const double xi = (double)i;
            const long o = (i - r0) * w;
            for (long j = 0; j < w; ++j) {
                const double yj = (double)j;
                u0[o + j] = std::exp(-sigma * ((xi * dx - x0) * (xi * dx - x0) +
                                               (yj * dx - y0) * (yj * dx - y0)));
                v1[o + j] = -ky * std::sin(kx * xi * dx) * std::cos(ky * yj * dx);
                v2[o + j] = kx * std::cos(kx * xi * dx) * std::sin(ky * yj * dx);
            }
        }
    };
    std::vector<std::thread> th;
    const long per = (r1 - r0 + nt - 1) / nt;
    for (int t = 0; t < nt; ++t) {
        long a = r0 + t * per, b = std::min(r1, a + per);
        if (a < b) th.emplace_back(rows, a, b);
    }
    for (auto &x : th) x.join();
    // zero boundary, multigrid.cpp:227-233 (row N, column 0 stays: the
    // reference's loops skip that corner)
    auto in = [&](long i) { return i >= r0 && i < r1; };
    for (long i = 0; i < N; ++i) {
        if (in(0)) u0[(0 - r0) * w + i] = 0.0;
        if (in(i)) u0[(i - r0) * w + N] = 0.0;
        if (in(N)) u0[(N - r0) * w + i + 1] = 0.0;
        if (in(i)) u0[(i - r0) * w] = 0.0;
    }
    return MGX_OK;
}

extern "C" int mgx_init_problem(double *u0, double *v1, double *v2, long N, int nthreads) {
    if (!u0 || !v1 || !v2 || N < 1) return fail(MGX_E_ARG, "mgx_init_problem: bad args");
    return init_rows(u0, v1, v2, N, 0, N + 1, nthreads);
}

extern "C" int mgx_init_problem_rows(double *u0, double *v1, double *v2, long N, long r0,
                                     long r1, int nthreads) {
    if (!u0 || !v1 || !v2 || N < 1 || r0 < 0 || r1 > N + 1 || r0 >= r1)
        return fail(MGX_E_ARG, "mgx_init_problem_rows: bad args");
    return init_rows(u0, v1, v2, N, r0, r1, nthreads);
}

// The reference's uT text writer (multigrid.cpp:269-284: fprintf "%d\t%d\t%f\n",
// i outer, j inner) for rows [r0, r1) held in `rows` ((r1-r0) x (N+1)), so a
// row-partitioned run writes its output block by block: rank r appends its
// owned rows in rank order and the file is byte-identical to the whole-grid
// writer.  Lines are formatted by nthreads threads, written in order.
extern "C" int mgx_write_uT(const char *path, const double *rows, long N, long r0, long r1,
                            int append, int nthreads) {
    if (!path || !rows || N < 1 || r0 < 0 || r1 > N + 1 || r0 > r1)
        return fail(MGX_E_ARG, "mgx_write_uT: bad args");
    FILE *f = fopen(path, append ? "ab" : "wb");
    if (!f) return fail(MGX_E_ARG, std::string("mgx_write_uT: cannot open ") + path);
    int nt = nthreads > 0 ? nthreads : (int)std::thread::hardware_concurrency();
    nt = std::max(1, std::min(nt, 64));
    const long w = N + 1, per = 8;   // rows per thread per batch
    std::vector<std::string> buf(nt);
    int rc = MGX_OK;
    for (long b0 = r0; b0 < r1 && rc == MGX_OK; b0 += per * nt) {
        auto fmt = [&](int t) {
            std::string &s = buf[t];
            s.clear();
            char line[400];   // "%f" of DBL_MAX is 316 characters
            const long a = b0 + t * per, e = std::min(r1, a + per);
            for (long i = a; i < e; ++i)
                for (long j = 0; j < w; ++j) {
                    const int k = snprintf(line, sizeof line, "%d\t%d\t%f\n", (int)i, (int)j,
                                           rows[(i - r0) * w + j]);
                    s.append(line, k);
                }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < nt; ++t) th.emplace_back(fmt, t);
        fmt(0);
        for (auto &x : th) x.join();
        for (int t = 0; t < nt && rc == MGX_OK; ++t)
            if (!buf[t].empty() && fwrite(buf[t].data(), 1, buf[t].size(), f) != buf[t].size())
                rc = fail(MGX_E_ARG, std::string("mgx_write_uT: write failed: ") + path);
    }
    if (fclose(f) != 0 && rc == MGX_OK) rc = fail(MGX_E_ARG, "mgx_write_uT: close failed");
    return rc;
}

// sepvel.h's exact rank-1 factorisation, for tests: v (rows x (n+1)) ==
// fl(a[i] * b[j]) bitwise -> 1 (a, b filled), else 0.  Host only.
extern "C" int mgx_factor_velocity(const double *v, long rows, long n, double smin, double *a,
                                   double *b) {
    if (!v || !a || !b || rows < 1 || n < 1) return fail(MGX_E_ARG, "mgx_factor_velocity: bad args");
    return mgxsep::factor_rank1(v, rows, n + 1, n + 1, smin, a, b) ? 1 : 0;
}

// The same on a field in device memory (vfactor.hip), row stride ld; a, b are
// device pointers too.
extern "C" int mgx_factor_velocity_device(const double *v, long rows, long n, long ld, double smin,
                                          double *a, double *b, int *factored) {
    if (!v || !a || !b || !factored || rows < 1 || n < 1 || ld < n + 1)
        return fail(MGX_E_ARG, "mgx_factor_velocity_device: bad args");
    *factored = 0;
    std::vector<double> ha((size_t)rows), hb((size_t)n + 1);
    hipError_t e = hipSuccess;
    const int r = mgxvf::factor_rank1_device(v, rows, n + 1, ld, smin, ha.data(), hb.data(),
                                             nullptr, nullptr, &e);
    if (r < 0)
        return fail(MGX_E_HIP, std::string("mgx_factor_velocity_device: ") + hipGetErrorString(e));
    if (r == 1) {
        HIPCHK(hipMemcpy(a, ha.data(), sizeof(double) * ha.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(b, hb.data(), sizeof(double) * hb.size(), hipMemcpyHostToDevice));
        *factored = 1;
    }
    return MGX_OK;
}

// whether the context's finest level holds velocity factors (its cross pass
// reads rhs and u only)
extern "C" int mgx_velocity_factored(mgx_ctx *c, int *factored) {
    if (!c || !factored) return fail(MGX_E_ARG, "mgx_velocity_factored: bad args");
    if (c->dist) {
        *factored = dist_velocity_mask(c);
        return MGX_OK;
    }
    int f = (!c->lv.empty() && c->lv[0].sa1) ? 1 : 0;
    for (size_t l = 1; l < c->lv.size() && l < 31; ++l)
        if (c->lv[l].vgen && mgxi::g_vgen) f |= 1 << l;
    *factored = f;
    return MGX_OK;
}

// ---- tuning knobs (process-wide)
extern "C" int mgx_set_tuning(const char *key, long value) {
    if (!key) return fail(MGX_E_ARG, "mgx_set_tuning: null key");
    ++mgxi::g_tuning_epoch;   // captured sub-cycles of the old settings are stale
    if (!strcmp(key, "graph_level")) {
        if (value < 0) return fail(MGX_E_ARG, "graph_level must be >= 0");
        mgxi::g_graph_level = value;
        return MGX_OK;
    }
    if (!strcmp(key, "tile_max_n")) {
        mgx::set_tile_max_n(value);
        return MGX_OK;
    }
    if (!strcmp(key, "cross_cycle")) {
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "cross_cycle must be 0 or 1");
        mgxi::g_cross_cycle = value;
        return MGX_OK;
    }
    if (!strcmp(key, "dist_overlap")) {
        if (value < -1 || value > 2) return fail(MGX_E_ARG, "dist_overlap must be -1, 0, 1 or 2");
        mgxi::g_dist_overlap = value;
        return MGX_OK;
    }
    if (!strcmp(key, "dist_local_side")) {
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "dist_local_side must be 0 or 1");
        mgxi::g_dist_local_side = value;
        return MGX_OK;
    }
    if (!strcmp(key, "coarse_fuse")) {
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "coarse_fuse must be 0 or 1");
        mgxi::g_coarse_fuse = value;
        return MGX_OK;
    }
    if (!strcmp(key, "wpair")) {
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "wpair must be 0 or 1");
        mgxi::g_wpair = value;
        return MGX_OK;
    }
    if (!strcmp(key, "dist_comm_chain")) {   // test hook (dist.hip)
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "dist_comm_chain must be 0 or 1");
        mgxi::g_dist_comm_chain = value;
        return MGX_OK;
    }
    if (!strcmp(key, "dist_min_rows")) {
        if (value < 16 || (value & 1)) return fail(MGX_E_ARG, "dist_min_rows must be even, >= 16");
        mgxi::g_dist_min_rows = value;
        return MGX_OK;
    }
    if (!strcmp(key, "xfast")) {
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "xfast must be 0 or 1");
        mgx::set_xfast(value);
        return MGX_OK;
    }
    if (!strcmp(key, "xpack")) {
        if (value < 0 || value > 2) return fail(MGX_E_ARG, "xpack must be 0, 1 or 2");
        mgxi::g_xpack = value;
        return MGX_OK;
    }
    if (!strcmp(key, "wpack")) {
        if (value < 0 || value > 3) return fail(MGX_E_ARG, "wpack must be 0, 1, 2 or 3");
        mgxi::g_wpack = value;
        return MGX_OK;
    }
    if (!strcmp(key, "tile32_min_n")) {
        if (value < 0) return fail(MGX_E_ARG, "tile32_min_n must be >= 0");
        mgx::set_tile32_min_n(value);
        return MGX_OK;
    }
    if (!strcmp(key, "tile_xcd")) {
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "tile_xcd must be 0 or 1");
        mgx::set_tile_xcd(value);
        return MGX_OK;
    }
    if (!strcmp(key, "march_order")) {
        if (value < 0 || value > 3) return fail(MGX_E_ARG, "march_order must be 0..3");
        mgx::set_march_order(value);
        return MGX_OK;
    }
    if (!strcmp(key, "march_min_rows")) {
        if (value < 8) return fail(MGX_E_ARG, "march_min_rows must be >= 8");
        mgx::set_march_min_rows(value);
        return MGX_OK;
    }
    if (!strcmp(key, "xtile_max_rows")) {
        if (value < 0) return fail(MGX_E_ARG, "xtile_max_rows must be >= 0");
        mgx::set_xtile_max_rows(value);
        return MGX_OK;
    }
    if (!strcmp(key, "step_cross")) {
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "step_cross must be 0 or 1");
        g_step_cross = value;
        return MGX_OK;
    }
    if (!strcmp(key, "post_only")) {
        if (value < -1) return fail(MGX_E_ARG, "post_only must be >= -1");
        mgxi::g_post_only = value;
        return MGX_OK;
    }
    if (!strcmp(key, "post_predict")) {
        if (value < -1) return fail(MGX_E_ARG, "post_predict must be >= -1");
        mgxi::g_post_predict = (double)value;
        return MGX_OK;
    }
    if (!strcmp(key, "march_seg")) {
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "march_seg must be 0 or 1");
        mgx::set_march_seg(value);
        return MGX_OK;
    }
    if (!strcmp(key, "step_fuse")) {
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "step_fuse must be 0 or 1");
        mgxi::g_step_fuse = value;
        return MGX_OK;
    }
    if (!strcmp(key, "coarse_lds")) {
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "coarse_lds must be 0 or 1");
        mgx::set_coarse_lds(value);
        return MGX_OK;
    }
    if (!strcmp(key, "sep_velocity")) {
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "sep_velocity must be 0 or 1");
        mgxi::g_sep_velocity = value;
        return MGX_OK;
    }
    if (!strcmp(key, "device_factor")) {
        if (value < 0 || value > 2) return fail(MGX_E_ARG, "device_factor must be 0, 1 or 2");
        mgxi::g_device_factor = value;
        return MGX_OK;
    }
    if (!strcmp(key, "vgen")) {
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "vgen must be 0 or 1");
        mgxi::g_vgen = value;
        return MGX_OK;
    }
    if (!strcmp(key, "source_sv")) {
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "source_sv must be 0 or 1");
        mgxi::g_source_sv = value;
        return MGX_OK;
    }
    if (!strcmp(key, "dense_rows")) {
        if (value < 0 || value > 65535) return fail(MGX_E_ARG, "dense_rows must be 0..65535");
        mgxi::g_dense_rows = value;
        return MGX_OK;
    }
    if (!strcmp(key, "dense_store")) {
        if (value < 0 || value > 2) return fail(MGX_E_ARG, "dense_store must be 0, 1 or 2");
        mgxi::g_dense_store = value;
        return MGX_OK;
    }
    if (!strcmp(key, "zero_rows")) {
        if (value != 0 && value != 1) return fail(MGX_E_ARG, "zero_rows must be 0 or 1");
        mgxi::g_zero_rows = value;
        return MGX_OK;
    }
    if (!strcmp(key, "march_tile_rows")) {
        if (value < 0) return fail(MGX_E_ARG, "march_tile_rows must be >= 0");
        mgx::set_march_tile_rows(value);
        return MGX_OK;
    }
    return fail(MGX_E_ARG, std::string("mgx_set_tuning: unknown key ") + key);
}
extern "C" int mgx_get_tuning(const char *key, long *value) {
    if (!key || !value) return fail(MGX_E_ARG, "mgx_get_tuning: null argument");
    if (!strcmp(key, "graph_level")) {
        *value = mgxi::g_graph_level;
        return MGX_OK;
    }
    if (!strcmp(key, "graph_captures") || !strcmp(key, "graph_replays")) {
        *value = key[6] == 'c' ? mgxi::g_graph_captures : mgxi::g_graph_replays;
        return MGX_OK;
    }
    if (!strcmp(key, "tile_max_n")) {
        *value = mgx::get_tile_max_n();
        return MGX_OK;
    }
    if (!strcmp(key, "cross_cycle")) {
        mgxi::cross_cycle_on();
        *value = mgxi::g_cross_cycle;
        return MGX_OK;
    }
    if (!strcmp(key, "dist_overlap")) {
        *value = mgxi::g_dist_overlap;
        return MGX_OK;
    }
    if (!strcmp(key, "dist_local_side")) {
        *value = mgxi::g_dist_local_side;
        return MGX_OK;
    }
    if (!strcmp(key, "dist_comm_chain")) {
        *value = mgxi::g_dist_comm_chain;
        return MGX_OK;
    }
    if (!strcmp(key, "coarse_fuse")) {
        *value = mgxi::g_coarse_fuse;
        return MGX_OK;
    }
    if (!strcmp(key, "wpair")) {
        *value = mgxi::g_wpair;
        return MGX_OK;
    }
    if (!strcmp(key, "dist_min_rows")) {
        *value = mgxi::g_dist_min_rows;
        return MGX_OK;
    }
    if (!strcmp(key, "xpack")) {
        *value = mgxi::g_xpack;
        return MGX_OK;
    }
    if (!strcmp(key, "wpack")) {
        *value = mgxi::g_wpack;
        return MGX_OK;
    }
    if (!strcmp(key, "xfast")) {
        *value = mgx::get_xfast();
        return MGX_OK;
    }
    if (!strcmp(key, "tile32_min_n")) {
        *value = mgx::get_tile32_min_n();
        return MGX_OK;
    }
    if (!strcmp(key, "tile_xcd")) {
        *value = mgx::get_tile_xcd();
        return MGX_OK;
    }
    if (!strcmp(key, "march_order")) {
        *value = mgx::get_march_order();
        return MGX_OK;
    }
    if (!strcmp(key, "march_min_rows")) {
        *value = mgx::get_march_min_rows();
        return MGX_OK;
    }
    if (!strcmp(key, "xtile_max_rows")) {
        *value = mgx::get_xtile_max_rows();
        return MGX_OK;
    }
    if (!strcmp(key, "step_cross")) {
        *value = g_step_cross;
        return MGX_OK;
    }
    if (!strcmp(key, "post_only")) {
        *value = mgxi::g_post_only;
        return MGX_OK;
    }
    if (!strcmp(key, "post_predict")) {
        *value = (long)mgxi::g_post_predict;
        return MGX_OK;
    }
    if (!strcmp(key, "march_seg")) {
        *value = mgx::get_march_seg();
        return MGX_OK;
    }
    if (!strcmp(key, "step_fuse")) {
        *value = mgxi::g_step_fuse;
        return MGX_OK;
    }
    if (!strcmp(key, "coarse_lds")) {
        *value = mgx::get_coarse_lds();
        return MGX_OK;
    }
    if (!strcmp(key, "sep_velocity")) {
        *value = mgxi::g_sep_velocity;
        return MGX_OK;
    }
    if (!strcmp(key, "device_factor")) {
        *value = mgxi::g_device_factor;
        return MGX_OK;
    }
    // (read-only, for measurements: the check-kernel launches of this thread's
    // last device factorisation and their summed device microseconds)
    if (!strcmp(key, "vfactor_rounds") || !strcmp(key, "vfactor_us")) {
        int rounds = 0;
        double ms = 0;
        mgxvf::last_stats(&rounds, &ms);
        *value = key[8] == 'r' ? (long)rounds : (long)(ms * 1e3);
        return MGX_OK;
    }
    // (read-only: the calling thread's last statistics call, mgx_field_stats*
    // / mgx_array_stats -- device microseconds of its reduction launches and
    // their compulsory bytes)
    if (!strcmp(key, "stats_us") || !strcmp(key, "stats_bytes")) {
        double us = 0, bytes = 0;
        mgxdiag::last_pass(&us, &bytes);
        *value = key[6] == 'u' ? (long)us : (long)bytes;
        return MGX_OK;
    }
    // (read-only: the same of the calling thread's last error pass,
    // mgx_step_error* / mgx_array_step_error)
    if (!strcmp(key, "errest_us") || !strcmp(key, "errest_bytes")) {
        double us = 0, bytes = 0;
        mgxerr::last_pass(&us, &bytes);
        *value = key[7] == 'u' ? (long)us : (long)bytes;
        return MGX_OK;
    }
    // (read-only: the same of the calling thread's last dense call,
    // mgx_dense_output* / mgx_dense_points* / mgx_array_dense)
    if (!strcmp(key, "dense_us") || !strcmp(key, "dense_bytes")) {
        double us = 0, bytes = 0;
        mgxdense::last_pass(&us, &bytes);
        *value = key[6] == 'u' ? (long)us : (long)bytes;
        return MGX_OK;
    }
    if (!strcmp(key, "dense_rows")) {
        *value = mgxi::g_dense_rows;
        return MGX_OK;
    }
    if (!strcmp(key, "dense_store")) {
        *value = mgxi::g_dense_store;
        return MGX_OK;
    }
    // (read-only: the device microseconds of the calling thread's last ring
    // write, mgx_set_boundary* now or consumed by a step)
    if (!strcmp(key, "boundary_us")) {
        *value = (long)mgxbc::last_us();
        return MGX_OK;
    }
    if (!strcmp(key, "vgen")) {
        *value = mgxi::g_vgen;
        return MGX_OK;
    }
    if (!strcmp(key, "source_sv")) {
        *value = mgxi::g_source_sv;
        return MGX_OK;
    }
    if (!strcmp(key, "zero_rows")) {
        *value = mgxi::g_zero_rows;
        return MGX_OK;
    }
    if (!strcmp(key, "march_tile_rows")) {
        *value = mgx::get_march_tile_rows();
        return MGX_OK;
    }
    return fail(MGX_E_ARG, std::string("mgx_get_tuning: unknown key ") + key);
}

// Streaming-bandwidth probe (a measured ceiling beside the spec).
extern "C" int mgx_stream_bandwidth(long bytes_per_stream, int nin, int reps, double *GBs) {
    if (bytes_per_stream < (1 << 20) || (nin != 1 && nin != 4) || reps < 1 || !GBs)
        return fail(MGX_E_ARG, "mgx_stream_bandwidth: bad args");
    const long n2 = bytes_per_stream / 16;
    const size_t bytes = (size_t)n2 * 16;
    double *buf[5] = {};
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = MGX_OK;
    int dev = 0, cus = 0;
    auto cleanup = [&]() {
        for (double *b : buf) (void)hipFree(b);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (s) (void)hipStreamDestroy(s);
    };
    for (int k = 0; k <= nin; ++k)
        if (hipMalloc(&buf[k], bytes) != hipSuccess ||
            hipMemset(buf[k], 0, bytes) != hipSuccess) {
            cleanup();
            return fail(MGX_E_HIP, "mgx_stream_bandwidth: alloc");
        }
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipStreamCreate(&s) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
        hipEventCreate(&e1) != hipSuccess) {
        cleanup();
        return fail(MGX_E_HIP, "mgx_stream_bandwidth: stream/events");
    }
    // one 16-B element per lane (kernels.hip k_stream)
    const int grid = (int)std::min<long>((n2 + 255) / 256, 1L << 30);
    double *a = buf[0], *b = buf[nin > 1 ? 1 : 0], *c = buf[nin > 1 ? 2 : 0],
           *d = buf[nin > 1 ? 3 : 0], *o = buf[nin];
    mgx::launch_stream(a, b, c, d, o, n2, nin, grid, s);   // warm-up
    (void)hipEventRecord(e0, s);
    for (int r = 0; r < reps; ++r) mgx::launch_stream(a, b, c, d, o, n2, nin, grid, s);
    (void)hipEventRecord(e1, s);
    float ms = 0.f;
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)
        rc = fail(MGX_E_HIP, "mgx_stream_bandwidth: timing");
    else
        *GBs = (double)bytes * (nin + 1) * reps / (ms * 1e-3) / 1e9;
    cleanup();
    return rc;
}

// tstep.hip -- the two-operator "rhs + initial norm" row march (tstep.h): the
// first pass of a step whose right-hand side and solve side use different k
// (mgx_set_time_step with theta != 1/2).
//
// Built with -ffp-contract=off like every other translation unit: rhs =
// fl(Bu + fl(cf * f)) and the residual against A u in the reference's term
// order, in either fp_mode.
#include "tstep.h"

#include "stencil.h"

#include <algorithm>

namespace mgxts {

using namespace mgx;

namespace {

// Row march, the frame of source.hip's k_rhs_source<NORM = true> (block = 256
// lanes = 512 columns, one column pair per lane, 16-B loads and stores; grid
// (strips, row groups) of res_grid): per row
//     rhs = B u            (rhs_point with cb, gs.cpp:44, k = kB)
//         (+ fl(cf * f))   (SRC 1: f a finest-level array; SRC 2: a separable
//                           source of `terms` terms formed in registers)
//     acc += (rhs - A u)^2 (res_point with ca, gs.cpp:75, k = kA)
// The two Coefs are kernel arguments (scalar registers); the velocity part of
// the four off-diagonal coefficients, fl(fl(-+v * h / 2) + nu), is the same for
// both and is formed once per point by the compiler, each scaled by its own rr.
//   SV:    v1 / v2 from their exact factors (sepvel.h), as in k_rhs_source.
//   SRC 2: the number of terms is a run-time argument (one instance for 1..4
//          terms, every branch on it wave-uniform); the column factors of the
//          first HOLD terms stay in registers for the whole march, the others
//          in LDS, a private slot per lane (written once before the march,
//          read back by the lane that wrote it: no barrier).  HOLD is 2, and 1
//          beside the velocity's column factors, so that every instance stays
//          within the 64 VGPRs of 8 waves per SIMD without scratch (at most 12
//          KiB of LDS a workgroup: eight workgroups a CU fit its 160 KiB).
//          f = t_0 (+ t_1 (+ t_2 (+ t_3))), t_r = fl(fa[r][i] * fb[r][j]), left
//          to right, each product and sum rounded: source.h's f bit for bit.
template <int SRC, bool SV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_rhs_norm2(
    const double *__restrict__ u, const double *__restrict__ v1, const double *__restrict__ v2,
    const double *__restrict__ sa1, const double *__restrict__ sb1,
    const double *__restrict__ sa2, const double *__restrict__ sb2,
    const double *__restrict__ f, const double *__restrict__ fa, const double *__restrict__ fb,
    int terms, double cf, int n, long pitch, Coef cb, Coef ca, int rows_per_group,
    double *__restrict__ out, double *__restrict__ partials, int r_first, int r_end) {
    __shared__ double lds[4];
    constexpr int HOLD = SV ? 1 : 2;
    __shared__ double2 gl[SRC == 2 ? (mgxsrc::kMaxTerms - HOLD) * 256 : 1];
    const int t = threadIdx.x, lane = t & 63;
    const long c0 = (long)blockIdx.x * 512 + 2 * t;
    const bool act = c0 <= n;
    const long i0 = r_first + (long)blockIdx.y * rows_per_group;
    const long i1 = std::min<long>(r_end, i0 + rows_per_group);
    double acc = 0.0;
    const double2 z2 = make_double2(0.0, 0.0);
    double2 un = z2, um = z2, us = z2;
    double2 b1 = z2, b2 = z2;
    double2 g[HOLD];
#pragma unroll
    for (int r = 0; r < HOLD; ++r) g[r] = z2;
    if (act && i0 < i1) {
        un = ld2(u + (i0 - 1) * pitch + c0);
        um = ld2(u + i0 * pitch + c0);
        if (SV) {   // (zero padded to the pitch: c0 + 1 < pitch)
            b1 = ld2(sb1 + c0);
            b2 = ld2(sb2 + c0);
        }
        if (SRC == 2) {
#pragma unroll
            for (int r = 0; r < mgxsrc::kMaxTerms; ++r) {
                if (r < terms) {
                    const double2 v = ld2(fb + r * pitch + c0);
                    if (r < HOLD)
                        g[r] = v;
                    else
                        gl[(r - HOLD) * 256 + t] = v;
                }
            }
        }
    }
    for (long i = i0; i < i1; ++i) {
        const long o = i * pitch;
        double2 x2 = z2, y2 = z2, s2 = z2;
        if (act) {
            us = ld2(u + o + pitch + c0);
            if (SRC == 2) {
                const long fw = n + 1;
                const double a0 = fa[i];
                s2 = make_double2(a0 * g[0].x, a0 * g[0].y);
#pragma unroll
                for (int r = 1; r < mgxsrc::kMaxTerms; ++r) {
                    if (r < terms) {
                        const double ar = fa[r * fw + i];
                        const double2 gr = r < HOLD ? g[r] : gl[(r - HOLD) * 256 + t];
                        const double tx = ar * gr.x, ty = ar * gr.y;
                        s2 = make_double2(s2.x + tx, s2.y + ty);
                    }
                }
            } else if (SRC == 1) {
                s2 = ld2s(f + o + c0);   // touched once per step
            }
            if (SV) {
                const double a1 = sa1[i], a2 = sa2[i];
                x2 = make_double2(a1 * b1.x, a1 * b1.y);
                y2 = make_double2(a2 * b2.x, a2 * b2.y);
            } else {
                x2 = ld2(v1 + o + c0);
                y2 = ld2(v2 + o + c0);
            }
        }
        // west of c0 and east of c0+1 from the neighbouring lanes' pairs
        double w = __shfl_up(um.y, 1, 64);
        double e = __shfl_down(um.x, 1, 64);
        if (lane == 0 && act && c0 >= 1) w = u[o + c0 - 1];
        if (lane == 63 && act && c0 + 2 <= n) e = u[o + c0 + 2];
        if (act) {
            const bool ok0 = c0 >= 1 && c0 <= n - 1, ok1 = c0 + 1 <= n - 1;
            // B u with kB (gs.cpp:44), then the source: fl(Bu + fl(cf * f))
            double2 r;
            r.x = rhs_point(x2.x, y2.x, um.x, un.x, w, us.x, um.y, cb);
            r.y = rhs_point(x2.y, y2.y, um.y, un.y, um.x, us.y, e, cb);
            if (SRC != 0) {
                const double sx = cf * s2.x, sy = cf * s2.y;
                r = make_double2(r.x + sx, r.y + sy);
            }
            if (ok0 && ok1) {
                st2(out + o + c0, r);
            } else {
                if (ok0) out[o + c0] = r.x;
                if (ok1) out[o + c0 + 1] = r.y;
            }
            // the residual against it with kA (gs.cpp:75)
            const double rx = res_point(r.x, x2.x, y2.x, um.x, un.x, w, us.x, um.y, ca);
            const double ry = res_point(r.y, x2.y, y2.y, um.y, un.y, um.x, us.y, e, ca);
            if (ok0) acc += rx * rx;
            if (ok1) acc += ry * ry;
        }
        un = um;
        um = us;
    }
    const double tot = block_sum(acc, lds);
    if (t == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

template <int SRC, bool SV>
void launch_inst(const mgxsrc::SrcArgs &a, const Coef &cA, dim3 g, int R, int f, int e,
                 hipStream_t s) {
    MGX_LAUNCH((k_rhs_norm2<SRC, SV>), g, dim3(256), s, a.u, a.v1, a.v2, a.sa1, a.sb1, a.sa2,
               a.sb2, a.f, a.fa, a.fb, a.terms, a.cf, (int)a.n, a.pitch, a.c, cA, R, a.rhs,
               a.partials, f, e);
}
template <bool SV>
void launch_form(const mgxsrc::SrcArgs &a, const Coef &cA, dim3 g, int R, int f, int e,
                 hipStream_t s) {
    if (a.terms > 0)
        launch_inst<2, SV>(a, cA, g, R, f, e, s);
    else if (a.f)
        launch_inst<1, SV>(a, cA, g, R, f, e, s);
    else
        launch_inst<0, SV>(a, cA, g, R, f, e, s);
}

}  // namespace

void launch_rhs_norm2(const mgxsrc::SrcArgs &a, const Coef &cA, hipStream_t s) {
    if (!a.partials || !a.norm_out || a.terms < 0 || a.terms > mgxsrc::kMaxTerms) return;
    int ra = a.ra, rb = a.rb;
    if (rb < 0) {
        ra = 0;
        rb = (int)a.n + 1;
    }
    const int f = std::max(1, ra), e = std::min((int)a.n, rb);   // interior rows [f, e)
    dim3 g;
    int R;
    mgxsrc::res_grid(a.n, e - f, g, R);   // launch_residual_norm's cut of the rows
    if (a.sa1 && a.sb1 && a.sa2 && a.sb2)
        launch_form<true>(a, cA, g, R, f, e, s);
    else
        launch_form<false>(a, cA, g, R, f, e, s);
    launch_norm_final(a.partials, (int)(g.x * g.y), a.norm_out, a.take_sqrt ? 1 : 0, s);
}

}  // namespace mgxts

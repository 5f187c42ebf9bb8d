// source.hip -- compute_rhs with a source term (source.h): one row march over
// the finest level and the raw op of the reference layout.
//
// Built with -ffp-contract=off like every other translation unit: the term is
// added as fl(Bu + fl(cf * f)), two roundings after the reference's Bu
// (gs.cpp:44), in either fp_mode.
#include "source.h"

#include "stencil.h"

#include <algorithm>

namespace mgxsrc {

using namespace mgx;

namespace {

// Row march, the frame of kernels.hip's k_res_march (block = 256 lanes = 512
// columns, one column pair per lane, 16-B loads and stores on the pitched
// arrays; grid (strips, row groups), rows [r_first + g*R, ...)).
//   NORM = false: rhs stored (k_res_march MODE 2 + the source);
//   NORM = true:  rhs stored AND the sum of squares of rhs - A u (MODE 3 + the
//                 source): the same grid, per-lane accumulation order,
//                 block_sum and partial layout as MODE 0, so k_norm_final gives
//                 bitwise the norm of launch_residual_norm on the stored rhs.
//   SV = true:    the velocity from its exact factors: v1[i][j] = fl(sa1[i] *
//                 sb1[j]) bitwise (sepvel.h's guarantee, the product the SV
//                 instances of k_xsmooth scale by h/2), v2 likewise; the
//                 column factors stay in registers for the whole march, the
//                 row factors are wave-uniform (scalar) loads.  u, f in and
//                 rhs out are the pass's only full streams.
//   SF = 0:       f is a finest-level array (one more full stream);
//   SF = 1..4:    f is a separable source of SF terms (source.h): the lane
//                 forms its column pair of f in registers,
//                     f = t_0 (+ t_1 (+ t_2 (+ t_3))) left to right,
//                     t_r = fl(fa[r][i] * fb[r][j]),
//                 each product and each sum rounded (no contraction), so f is
//                 bitwise the array numpy builds from the factors.  The fb
//                 pairs of the lane's two columns stay in registers for the
//                 whole march like sb1 / sb2 (fb[r] = fb + r*pitch, zero
//                 padded; one instance keeps two of them in LDS: HOLD below),
//                 the fa[r][i] (fa + r*(n+1)) are wave-uniform loads per row
//                 like sa1[i].  No f stream.  (waves_per_eu 8: every instance
//                 within the 64 VGPRs of 8 waves per SIMD, none with scratch.)
template <bool NORM, bool SV, int SF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_rhs_source(
    const double *__restrict__ u, const double *__restrict__ v1, const double *__restrict__ v2,
    const double *__restrict__ sa1, const double *__restrict__ sb1,
    const double *__restrict__ sa2, const double *__restrict__ sb2,
    const double *__restrict__ f, const double *__restrict__ fa, const double *__restrict__ fb,
    double cf, int n, long pitch, Coef c, int rows_per_group, double *__restrict__ out,
    double *__restrict__ partials, int r_first, int r_end) {
    __shared__ double lds[4];
    const int t = threadIdx.x, lane = t & 63;
    const long c0 = (long)blockIdx.x * 512 + 2 * t;
    const bool act = c0 <= n;
    const long i0 = r_first + (long)blockIdx.y * rows_per_group;
    const long i1 = std::min<long>(r_end, i0 + rows_per_group);
    double acc = 0.0;
    const double2 z2 = make_double2(0.0, 0.0);
    double2 un = z2, um = z2, us = z2;
    double2 b1 = z2, b2 = z2;
    // the separable source's column factors: HOLD of them stay in registers
    // for the whole march -- all of them, except in the one instance that would
    // not fit the 64 VGPRs of 8 waves per SIMD (norm + velocity factors + four
    // terms: 70 VGPRs holding all).  That one holds two in registers and the
    // other two in LDS, a private slot per lane (written once before the
    // march, read back per row by the lane that wrote it: no barrier).
    constexpr int HOLD = (NORM && SV && SF > 3) ? 2 : SF;
    constexpr int OVER = SF - HOLD;
    __shared__ double2 gl[(OVER > 0 ? OVER : 1) * 256];
    double2 g[SF > 0 ? SF : 1];
#pragma unroll
    for (int r = 0; r < SF; ++r) g[r] = z2;
    if (act && i0 < i1) {
        un = ld2(u + (i0 - 1) * pitch + c0);
        um = ld2(u + i0 * pitch + c0);
        if (SV) {   // (zero padded to the pitch: c0 + 1 < pitch)
            b1 = ld2(sb1 + c0);
            b2 = ld2(sb2 + c0);
        }
#pragma unroll
        for (int r = 0; r < HOLD; ++r) g[r] = ld2(fb + r * pitch + c0);
#pragma unroll
        for (int r = HOLD; r < SF; ++r) gl[(r - HOLD) * 256 + t] = ld2(fb + r * pitch + c0);
    }
    for (long i = i0; i < i1; ++i) {
        const long o = i * pitch;
        double2 x2 = z2, y2 = z2, s2 = z2;
        if (act) {
            us = ld2(u + o + pitch + c0);
            if (SF > 0) {
                const double a0 = fa[i];
                s2 = make_double2(a0 * g[0].x, a0 * g[0].y);
#pragma unroll
                for (int r = 1; r < SF; ++r) {
                    const double ar = fa[r * (long)(n + 1) + i];
                    const double2 gr = r < HOLD ? g[r] : gl[(r - HOLD) * 256 + t];
                    const double tx = ar * gr.x, ty = ar * gr.y;
                    s2 = make_double2(s2.x + tx, s2.y + ty);
                }
            } else {
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
            // Bu (gs.cpp:44), then the source: fl(Bu + fl(cf * f))
            const double bx = rhs_point(x2.x, y2.x, um.x, un.x, w, us.x, um.y, c);
            const double by = rhs_point(x2.y, y2.y, um.y, un.y, um.x, us.y, e, c);
            const double sx = cf * s2.x, sy = cf * s2.y;
            const double2 r = make_double2(bx + sx, by + sy);
            if (ok0 && ok1) {
                st2(out + o + c0, r);
            } else {
                if (ok0) out[o + c0] = r.x;
                if (ok1) out[o + c0 + 1] = r.y;
            }
            if (NORM) {   // the residual against it (gs.cpp:75)
                const double rx = res_point(r.x, x2.x, y2.x, um.x, un.x, w, us.x, um.y, c);
                const double ry = res_point(r.y, x2.y, y2.y, um.y, un.y, um.x, us.y, e, c);
                if (ok0) acc += rx * rx;
                if (ok1) acc += ry * ry;
            }
        }
        un = um;
        um = us;
    }
    if (NORM) {
        const double tot = block_sum(acc, lds);
        if (t == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = tot;
    }
}

// reference layout: one lane per point, pitch n+1 (rows only 8-B aligned),
// the frame of k_raw_rhs
__global__ __launch_bounds__(256) void k_raw_rhs_source(double *rhs, const double *u,
                                                        const double *v1, const double *v2,
                                                        const double *f, double cf, long n,
                                                        Coef c) {
    const long w = n + 1;
    const long j = 1 + (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    for (long i = 1 + blockIdx.y; i < n; i += gridDim.y) {
        const long p = i * w + j;
        const double b = rhs_point(v1[p], v2[p], u[p], u[p - w], u[p - 1], u[p + w], u[p + 1], c);
        const double s = cf * f[p];
        rhs[p] = b + s;
    }
}

// the same with a separable source: fa, fb are terms x (n+1), term-major
__global__ __launch_bounds__(256) void k_raw_rhs_source_sep(double *rhs, const double *u,
                                                            const double *v1, const double *v2,
                                                            int terms, const double *fa,
                                                            const double *fb, double cf, long n,
                                                            Coef c) {
    const long w = n + 1;
    const long j = 1 + (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    for (long i = 1 + blockIdx.y; i < n; i += gridDim.y) {
        const long p = i * w + j;
        const double b = rhs_point(v1[p], v2[p], u[p], u[p - w], u[p - 1], u[p + w], u[p + 1], c);
        double f = fa[i] * fb[j];
        for (int r = 1; r < terms; ++r) {
            const double t = fa[r * w + i] * fb[r * w + j];
            f = f + t;
        }
        const double s = cf * f;
        rhs[p] = b + s;
    }
}

template <bool NORM, bool SV, int SF>
void launch_inst(const SrcArgs &a, dim3 g, int R, int f, int e, hipStream_t s) {
    MGX_LAUNCH((k_rhs_source<NORM, SV, SF>), g, dim3(256), s, a.u, a.v1, a.v2, a.sa1, a.sb1, a.sa2,
               a.sb2, a.f, a.fa, a.fb, a.cf, (int)a.n, a.pitch, a.c, R, a.rhs, a.partials, f, e);
}
// the instance of the source's form: a field (terms 0) or 1..4 separable terms
template <bool NORM, bool SV>
void launch_form(const SrcArgs &a, dim3 g, int R, int f, int e, hipStream_t s) {
    switch (a.terms) {
        case 0: launch_inst<NORM, SV, 0>(a, g, R, f, e, s); break;
        case 1: launch_inst<NORM, SV, 1>(a, g, R, f, e, s); break;
        case 2: launch_inst<NORM, SV, 2>(a, g, R, f, e, s); break;
        case 3: launch_inst<NORM, SV, 3>(a, g, R, f, e, s); break;
        default: launch_inst<NORM, SV, 4>(a, g, R, f, e, s); break;
    }
}

}  // namespace

// kernels.hip's res_grid: the grid of every k_res_march launch (the norm
// instance must cut the rows exactly as launch_residual_norm does)
void res_grid(long n, long rows, dim3 &g, int &R) {
    const unsigned strips = cdiv(n + 1, 512);
    rows = std::max<long>(rows, 1);
    const long want = std::max<long>(1, 4096 / (long)strips);
    R = (int)std::max<long>(8, (rows + want - 1) / want);
    g = dim3(strips, cdiv(rows, R));
}

void launch_rhs_source(const SrcArgs &a, hipStream_t s) {
    int ra = a.ra, rb = a.rb;
    if (rb < 0) {
        ra = 0;
        rb = (int)a.n + 1;
    }
    const int f = std::max(1, ra), e = std::min((int)a.n, rb);   // interior rows [f, e)
    dim3 g;
    int R;
    res_grid(a.n, e - f, g, R);
    const bool sv = a.sa1 && a.sb1 && a.sa2 && a.sb2;
    const bool norm = a.partials != nullptr;
    if (norm) {
        if (sv)
            launch_form<true, true>(a, g, R, f, e, s);
        else
            launch_form<true, false>(a, g, R, f, e, s);
        launch_norm_final(a.partials, (int)(g.x * g.y), a.norm_out, a.take_sqrt ? 1 : 0, s);
    } else {
        if (sv)
            launch_form<false, true>(a, g, R, f, e, s);
        else
            launch_form<false, false>(a, g, R, f, e, s);
    }
}

void launch_raw_rhs_source(double *rhs, const double *u, const double *v1, const double *v2,
                           const double *f, double cf, long n, Coef c, hipStream_t s) {
    if (n < 2) return;
    // (gridDim.y capped as kernels.hip's raw ops cap it; the rows grid-stride)
    const unsigned gy = (unsigned)std::max<long>(1, std::min<long>(n - 1, 32768));
    MGX_LAUNCH(k_raw_rhs_source, dim3(cdiv(n - 1, 256), gy), dim3(256), s, rhs, u, v1, v2, f, cf, n,
               c);
}

void launch_raw_rhs_source_sep(double *rhs, const double *u, const double *v1, const double *v2,
                               int terms, const double *fa, const double *fb, double cf, long n,
                               Coef c, hipStream_t s) {
    if (n < 2 || terms < 1 || terms > kMaxTerms) return;
    const unsigned gy = (unsigned)std::max<long>(1, std::min<long>(n - 1, 32768));
    MGX_LAUNCH(k_raw_rhs_source_sep, dim3(cdiv(n - 1, 256), gy), dim3(256), s, rhs, u, v1, v2,
               terms, fa, fb, cf, n, c);
}

}  // namespace mgxsrc

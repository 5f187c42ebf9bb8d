// bdf.hip -- the "rhs + history + initial norm" row march of a variable-step
// BDF2 step (bdf.h): rhs = b0 u - b1 h (+ c f), h <- u, |rhs - A(kA) u|.
//
// Built with -ffp-contract=off like every other translation unit: each product
// and each sum of the right-hand side is rounded, and the residual against
// A u keeps the reference's term order, in either fp_mode.
#include "bdf.h"

#include "stencil.h"

#include <algorithm>

namespace mgxbdf {

using namespace mgx;

Coefs coefficients(double dt, double dt_prev) {
    const double w = dt / dt_prev;
    const double p = 1.0 + w;
    const double q = 1.0 + 2.0 * w;
    Coefs k;
    k.g = p / q;
    k.b0 = (p * p) / q;
    k.b1 = (w * w) / q;
    k.kA = (2.0 * k.g) * dt;
    return k;
}

namespace {

// Row march, the frame of tstep.hip's k_rhs_norm2 (block = 256 lanes = 512
// columns, one column pair per lane, 16-B loads and stores; grid (strips, row
// groups) of res_grid): per row
//     hm  = h(i, .)          (u^(n-1))
//     h(i, .) = u(i, .)      (the row the lane holds: same lane, same address)
//     rhs = fl(fl(b0 u) - fl(b1 hm))
//         (+ fl(cf * f))     (SRC 1: f a finest-level array; SRC 2: a separable
//                             source of `terms` terms formed in registers, as
//                             in k_rhs_norm2: HOLD column factors in registers,
//                             the others in a private LDS slot per lane)
//     acc += (rhs - A u)^2   (res_point with ca, gs.cpp:75, k = kA)
// Every row of h is written by exactly one row group: the interior rows
// [r_first, r_end) by the group that marches them, row r_first - 1 (edges & 1:
// the grid's row 0) from the `un` of the first group and row r_end (edges & 2:
// the grid's row n) from the last row the last group loaded.  Whole pairs are stored, so the ring's columns and the zero padding
// behind column n travel with their rows.  u is only read.
// hin is where u^(n-1) is read and h where u^n is stored: the same address with
// a history of depth 1, the two arrays of depth 2 (mgx_set_history_depth) --
// so neither is __restrict__.  Only the lane that stores a pair has read it.
template <int SRC, bool SV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_rhs_norm_bdf(
    const double *__restrict__ u, const double *hin, double *h, const double *__restrict__ v1,
    const double *__restrict__ v2, const double *__restrict__ sa1, const double *__restrict__ sb1,
    const double *__restrict__ sa2, const double *__restrict__ sb2,
    const double *__restrict__ f, const double *__restrict__ fa, const double *__restrict__ fb,
    int terms, double cf, double b0, double b1, int n, long pitch, Coef ca, int rows_per_group,
    double *__restrict__ out, double *__restrict__ partials, int r_first, int r_end, int edges) {
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
    double2 d1 = z2, d2 = z2;
    double2 g[HOLD];
#pragma unroll
    for (int r = 0; r < HOLD; ++r) g[r] = z2;
    if (act && i0 < i1) {
        un = ld2(u + (i0 - 1) * pitch + c0);
        um = ld2(u + i0 * pitch + c0);
        if (blockIdx.y == 0 && (edges & 1)) st2(h + (i0 - 1) * pitch + c0, un);
        if (SV) {   // (zero padded to the pitch: c0 + 1 < pitch)
            d1 = ld2(sb1 + c0);
            d2 = ld2(sb2 + c0);
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
        double2 x2 = z2, y2 = z2, s2 = z2, hm = z2;
        if (act) {
            us = ld2(u + o + pitch + c0);
            hm = ld2(hin + o + c0);   // u^(n-1): read once, then replaced (hin == h)
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
                x2 = make_double2(a1 * d1.x, a1 * d1.y);
                y2 = make_double2(a2 * d2.x, a2 * d2.y);
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
            // (hm is in registers: the load above has returned before this store issues)
            st2(h + o + c0, um);
            double2 r;
            {
                const double px = b0 * um.x, py = b0 * um.y;
                const double qx = b1 * hm.x, qy = b1 * hm.y;
                r = make_double2(px - qx, py - qy);
            }
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
    // um holds row i1: the grid's last row where the march ends below it
    if (act && i0 < i1 && blockIdx.y == gridDim.y - 1 && (edges & 2)) st2(h + i1 * pitch + c0, um);
    const double tot = block_sum(acc, lds);
    if (t == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

template <int SRC, bool SV>
void launch_inst(const mgxsrc::SrcArgs &a, const double *hin, double *h, double b0, double b1,
                 dim3 g, int R, int f, int e, int edges, hipStream_t s) {
    MGX_LAUNCH((k_rhs_norm_bdf<SRC, SV>), g, dim3(256), s, a.u, hin, h, a.v1, a.v2, a.sa1, a.sb1,
               a.sa2, a.sb2, a.f, a.fa, a.fb, a.terms, a.cf, b0, b1, (int)a.n, a.pitch, a.c, R,
               a.rhs, a.partials, f, e, edges);
}
template <bool SV>
void launch_form(const mgxsrc::SrcArgs &a, const double *hin, double *h, double b0, double b1,
                 dim3 g, int R, int f, int e, int edges, hipStream_t s) {
    if (a.terms > 0)
        launch_inst<2, SV>(a, hin, h, b0, b1, g, R, f, e, edges, s);
    else if (a.f)
        launch_inst<1, SV>(a, hin, h, b0, b1, g, R, f, e, edges, s);
    else
        launch_inst<0, SV>(a, hin, h, b0, b1, g, R, f, e, edges, s);
}

// the frame of k_raw_rhs_source
__global__ __launch_bounds__(256) void k_raw_rhs_bdf(double *rhs, const double *u, const double *h,
                                                     long n, double b0, double b1, const double *f,
                                                     double c) {
    const long w = n + 1;
    const long j = 1 + (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    for (long i = 1 + blockIdx.y; i < n; i += gridDim.y) {
        const long p = i * w + j;
        const double a = b0 * u[p];
        const double b = b1 * h[p];
        double r = a - b;
        if (f) {
            const double s = c * f[p];
            r = r + s;
        }
        rhs[p] = r;
    }
}

}  // namespace

void launch_rhs_norm_bdf(const mgxsrc::SrcArgs &a, const double *hin, double *h, double b0,
                         double b1, hipStream_t s) {
    if (!a.partials || !a.norm_out || !h || !hin || a.terms < 0 || a.terms > mgxsrc::kMaxTerms)
        return;
    int ra = a.ra, rb = a.rb;
    if (rb < 0) {
        ra = 0;
        rb = (int)a.n + 1;
    }
    const int f = std::max(1, ra), e = std::min((int)a.n, rb);   // interior rows [f, e)
    if (e <= f) return;
    // the rows of [ra, rb) outside the interior: the grid's row 0 and row n
    const int edges = (f - 1 >= ra ? 1 : 0) | (e < rb ? 2 : 0);
    dim3 g;
    int R;
    mgxsrc::res_grid(a.n, e - f, g, R);   // launch_residual_norm's cut of the rows
    if (a.sa1 && a.sb1 && a.sa2 && a.sb2)
        launch_form<true>(a, hin, h, b0, b1, g, R, f, e, edges, s);
    else
        launch_form<false>(a, hin, h, b0, b1, g, R, f, e, edges, s);
    launch_norm_final(a.partials, (int)(g.x * g.y), a.norm_out, a.take_sqrt ? 1 : 0, s);
}

void launch_raw_rhs_bdf(double *rhs, const double *u, const double *h, long n, double b0,
                        double b1, const double *f, double c, hipStream_t s) {
    if (n < 2) return;
    // (gridDim.y capped as kernels.hip's raw ops cap it; the rows grid-stride)
    const unsigned gy = (unsigned)std::max<long>(1, std::min<long>(n - 1, 32768));
    MGX_LAUNCH(k_raw_rhs_bdf, dim3(cdiv(n - 1, 256), gy), dim3(256), s, rhs, u, h, n, b0, b1, f, c);
}

}  // namespace mgxbdf

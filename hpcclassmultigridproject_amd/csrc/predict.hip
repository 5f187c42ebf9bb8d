// predict.hip -- the "rhs + guess + two norms" row march of a BDF2 step with a
// predicted start (predict.h): rhs = b0 u - b1 h (+ c f), g = the interpolant
// through u, h (, h2) one step ahead, |rhs - A(kA) u| and |rhs - A(kA) g|.
//
// Built with -ffp-contract=off like every other translation unit: each product
// and each sum of the right-hand side and of the guess is rounded, and both
// residuals keep the reference's term order, in either fp_mode.
#include "predict.h"

#include "stencil.h"

#include <algorithm>

namespace mgxpred {

using namespace mgx;

namespace {

struct W {
    double w0, w1, w2;
};

// dense.hip's point formula (E + 1 arrays)
template <int E>
__device__ __forceinline__ double gpoint(double u, double h, double h2, const W &w) {
    const double a = w.w0 * u;
    const double b = w.w1 * h;
    const double ab = a + b;
    if (E == 1) return ab;
    const double c = w.w2 * h2;
    return ab + c;
}
// a column pair of g: the formula where the point is interior, u's bits elsewhere
// (the ring, and the padding behind column n)
template <int E>
__device__ __forceinline__ double2 gpair(double2 u, double2 h, double2 h2, const W &w, bool in0,
                                         bool in1) {
    return make_double2(in0 ? gpoint<E>(u.x, h.x, h2.x, w) : u.x,
                        in1 ? gpoint<E>(u.y, h.y, h2.y, w) : u.y);
}

// Row march, the frame of bdf.hip's k_rhs_norm_bdf (block = 256 lanes = 512
// columns, one column pair per lane, 16-B loads and stores; grid (strips, row
// groups) of res_grid over the interior rows [1, n)): per row i
//     us, hs (, h2s) = row i+1 of u, h (, h2);  gs = row i+1 of g, formed at once
//     rhs(i, .) = fl(fl(b0 u) - fl(b1 h)) (+ fl(cf * f))      k_rhs_norm_bdf's
//     g(i, .) stored as a whole pair (ring and padding columns: u's)
//     acc0 += (rhs - A u)^2,  acc1 += (rhs - A g)^2           (res_point, k = kA)
// with a three-row window of u and one of g, and h's row i.  Lane 0's west and
// lane 63's east neighbours are scalar loads of u, h (, h2) with the same
// formula; everywhere else they come from the neighbouring lanes' pairs.
// Every row of gout is stored by exactly one row group: the interior rows by the
// group that marches them, row 0 by the first and row n by the last.  A group
// recomputes the rows of g above and below its own from u, h (, h2) -- the same
// operations on the same operands as the group that stores them.  Nothing the
// launch writes (rhs, gout, partials) is read by it.
template <int SRC, bool SV, int E>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_predict_bdf(
    const double *__restrict__ u, const double *__restrict__ h, const double *__restrict__ h2,
    double *__restrict__ gout, const double *__restrict__ v1, const double *__restrict__ v2,
    const double *__restrict__ sa1, const double *__restrict__ sb1,
    const double *__restrict__ sa2, const double *__restrict__ sb2,
    const double *__restrict__ f, const double *__restrict__ fa, const double *__restrict__ fb,
    int terms, double cf, double b0, double b1, W wt, int n, long pitch, Coef ca,
    int rows_per_group, double *__restrict__ out, double *__restrict__ partials, long pstride) {
    __shared__ double lds0[4], lds1[4];
    constexpr int HOLD = SV ? 1 : 2;
    __shared__ double2 gl[SRC == 2 ? (mgxsrc::kMaxTerms - HOLD) * 256 : 1];
    const int t = threadIdx.x, lane = t & 63;
    const long c0 = (long)blockIdx.x * 512 + 2 * t;
    const bool act = c0 <= n;
    const bool ok0 = c0 >= 1 && c0 <= n - 1, ok1 = c0 + 1 <= n - 1;   // interior columns
    const long i0 = 1 + (long)blockIdx.y * rows_per_group;
    const long i1 = std::min<long>(n, i0 + rows_per_group);
    double acc0 = 0.0, acc1 = 0.0;
    const double2 z2 = make_double2(0.0, 0.0);
    double2 un = z2, um = z2, us = z2;
    double2 gn = z2, gm = z2, gs = z2;
    double2 hm = z2;
    double2 d1 = z2, d2 = z2;
    double2 g[HOLD];
#pragma unroll
    for (int r = 0; r < HOLD; ++r) g[r] = z2;
    if (act && i0 < i1) {
        const long oa = (i0 - 1) * pitch + c0, ob = i0 * pitch + c0;
        un = ld2(u + oa);
        um = ld2(u + ob);
        const double2 hn = ld2(h + oa);
        hm = ld2(h + ob);
        double2 kn = z2, km = z2;
        if (E == 2) {
            kn = ld2(h2 + oa);
            km = ld2(h2 + ob);
        }
        const bool rin = i0 - 1 >= 1;   // (row i0 is interior)
        gn = gpair<E>(un, hn, kn, wt, rin && ok0, rin && ok1);
        gm = gpair<E>(um, hm, km, wt, ok0, ok1);
        if (blockIdx.y == 0) st2(gout + oa, gn);   // the grid's row 0: u's
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
        double2 x2 = z2, y2 = z2, s2 = z2;
        double2 hs = z2;
        if (act) {
            us = ld2(u + o + pitch + c0);
            hs = ld2(h + o + pitch + c0);
            double2 ks = z2;
            if (E == 2) ks = ld2(h2 + o + pitch + c0);
            const bool rin = i + 1 <= n - 1;
            gs = gpair<E>(us, hs, ks, wt, rin && ok0, rin && ok1);
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
        double wg = __shfl_up(gm.y, 1, 64);
        double eg = __shfl_down(gm.x, 1, 64);
        if (lane == 0 && act && c0 >= 1) {   // column c0 - 1 of an interior row: interior
            const long p = o + c0 - 1;
            w = u[p];
            wg = gpoint<E>(w, h[p], E == 2 ? h2[p] : 0.0, wt);
        }
        if (lane == 63 && act && c0 + 2 <= n) {
            const long p = o + c0 + 2;
            e = u[p];
            eg = c0 + 2 <= n - 1 ? gpoint<E>(e, h[p], E == 2 ? h2[p] : 0.0, wt) : e;
        }
        if (act) {
            st2(gout + o + c0, gm);
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
            // the two residuals against it with kA (gs.cpp:75)
            const double rx = res_point(r.x, x2.x, y2.x, um.x, un.x, w, us.x, um.y, ca);
            const double ry = res_point(r.y, x2.y, y2.y, um.y, un.y, um.x, us.y, e, ca);
            const double px = res_point(r.x, x2.x, y2.x, gm.x, gn.x, wg, gs.x, gm.y, ca);
            const double py = res_point(r.y, x2.y, y2.y, gm.y, gn.y, gm.x, gs.y, eg, ca);
            if (ok0) {
                acc0 += rx * rx;
                acc1 += px * px;
            }
            if (ok1) {
                acc0 += ry * ry;
                acc1 += py * py;
            }
        }
        un = um;
        um = us;
        gn = gm;
        gm = gs;
        hm = hs;
    }
    // gm holds row i1: the grid's row n (u's bits) where the march ends below it
    if (act && i0 < i1 && blockIdx.y == gridDim.y - 1) st2(gout + i1 * pitch + c0, gm);
    const double tot0 = block_sum(acc0, lds0);
    const double tot1 = block_sum(acc1, lds1);
    if (t == 0) {
        const long b = (long)blockIdx.y * gridDim.x + blockIdx.x;
        partials[b] = tot0;
        partials[pstride + b] = tot1;
    }
}

template <int SRC, bool SV, int E>
void launch_inst(const mgxsrc::SrcArgs &a, const double *h, const double *h2, const W &w,
                 double *gout, double b0, double b1, dim3 g, int R, hipStream_t s) {
    MGX_LAUNCH((k_predict_bdf<SRC, SV, E>), g, dim3(256), s, a.u, h, h2, gout, a.v1, a.v2, a.sa1,
               a.sb1, a.sa2, a.sb2, a.f, a.fa, a.fb, a.terms, a.cf, b0, b1, w, (int)a.n, a.pitch,
               a.c, R, a.rhs, a.partials, (long)norm_partials_size());
}
template <bool SV, int E>
void launch_form(const mgxsrc::SrcArgs &a, const double *h, const double *h2, const W &w,
                 double *gout, double b0, double b1, dim3 g, int R, hipStream_t s) {
    if (a.terms > 0)
        launch_inst<2, SV, E>(a, h, h2, w, gout, b0, b1, g, R, s);
    else if (a.f)
        launch_inst<1, SV, E>(a, h, h2, w, gout, b0, b1, g, R, s);
    else
        launch_inst<0, SV, E>(a, h, h2, w, gout, b0, b1, g, R, s);
}
template <int E>
void launch_order(const mgxsrc::SrcArgs &a, const double *h, const double *h2, const W &w,
                  double *gout, double b0, double b1, dim3 g, int R, hipStream_t s) {
    if (a.sa1 && a.sb1 && a.sa2 && a.sb2)
        launch_form<true, E>(a, h, h2, w, gout, b0, b1, g, R, s);
    else
        launch_form<false, E>(a, h, h2, w, gout, b0, b1, g, R, s);
}

}  // namespace

void launch_predict_bdf(const mgxsrc::SrcArgs &a, const double *h, const double *h2, int order,
                        const double w[3], double *gout, double b0, double b1, hipStream_t s) {
    if (!a.partials || !a.norm_out || !h || !gout || a.terms < 0 || a.terms > mgxsrc::kMaxTerms)
        return;
    if ((order != 1 && order != 2) || (order == 2 && !h2) || a.n < 2) return;
    dim3 g;
    int R;
    mgxsrc::res_grid(a.n, a.n - 1, g, R);   // launch_residual_norm's cut of the rows
    const W wt{w[0], w[1], w[2]};
    if (order == 2)
        launch_order<2>(a, h, h2, wt, gout, b0, b1, g, R, s);
    else
        launch_order<1>(a, h, nullptr, wt, gout, b0, b1, g, R, s);
    const int nb = (int)(g.x * g.y);
    launch_norm_final(a.partials, nb, a.norm_out, 1, s);
    launch_norm_final(a.partials + norm_partials_size(), nb, a.norm_out + 1, 1, s);
}

}  // namespace mgxpred

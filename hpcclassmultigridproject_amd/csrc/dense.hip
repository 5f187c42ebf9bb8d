// dense.hip -- dense output: the interpolant through u, h and h2 (dense.h).
//
// Built with -ffp-contract=off like every other translation unit: each product
// and each sum of the point formula is rounded once.
#include "dense.h"

#include "stencil.h"

#include <algorithm>
#include <cmath>

namespace mgxdense {

using namespace mgx;

int weights(int order, double tau, double dt1, double dt2, double w[3]) {
    if (order < 0 || order > 2) return 1;
    if (!std::isfinite(tau)) return 2;
    if (order >= 1 && !(std::isfinite(dt1) && dt1 > 0)) return 3;
    if (order == 2 && !(std::isfinite(dt2) && dt2 > 0)) return 4;
    if (order == 0) {
        w[0] = 1.0;
        w[1] = w[2] = 0.0;
    } else if (order == 1) {
        const double mt = 0.0 - tau;
        w[1] = mt / dt1;
        w[0] = 1.0 - w[1];
        w[2] = 0.0;
    } else {
        const double s = dt1 + dt2;
        const double a = tau + dt1;
        const double b = tau + s;
        const double mt = 0.0 - tau;
        const double n0 = a * b, d0 = dt1 * s;
        const double n1 = mt * b, d1 = dt1 * dt2;
        const double n2 = tau * a, d2 = s * dt2;
        w[0] = n0 / d0;
        w[1] = n1 / d1;
        w[2] = n2 / d2;
    }
    return 0;
}

namespace {

struct W {
    double w0, w1, w2;
};

// the point formula; LV = 1 returns u's bits
template <int LV>
__device__ __forceinline__ double point(double u, double h, double h2, const W &w) {
    if (LV == 1) return u;
    const double a = w.w0 * u;
    const double b = w.w1 * h;
    const double ab = a + b;
    if (LV == 2) return ab;
    const double c = w.w2 * h2;
    return ab + c;
}

// A column pair into a row of the reference layout.  The row pitch n + 1 is
// odd, so the pair's 16-byte alignment alternates with the row's parity.
// ST 0 / 1: the aligned rows take one 16-byte store, the others (and a pair cut
// at column n) 8-byte stores -- a wave writes its 1 KB contiguously either way;
// ST 1 makes them non-temporal.  ST 2: one 16-byte store on every row, which on
// the other rows is only 8-byte aligned (the form of stencil.h's ldu2).  The
// branch is uniform over a row but for the cut pair.
template <int ST>
__device__ __forceinline__ void store_pair(double *p, double2 v, bool has1) {
    typedef double d2a8 __attribute__((ext_vector_type(2), aligned(8)));
    const bool aligned = (reinterpret_cast<unsigned long>(p) & 15ul) == 0;
    if (has1 && (ST == 2 || aligned)) {
        const mgx_d2v q = {v.x, v.y};
        if (ST == 1)
            __builtin_nontemporal_store(q, reinterpret_cast<mgx_d2v *>(p));
        else if (ST == 2)
            *reinterpret_cast<d2a8 *>(p) = q;
        else
            *reinterpret_cast<mgx_d2v *>(p) = q;
    } else {
        if (ST == 1) {
            __builtin_nontemporal_store(v.x, p);
            if (has1) __builtin_nontemporal_store(v.y, p + 1);
        } else {
            p[0] = v.x;
            if (has1) p[1] = v.y;
        }
    }
}

// Row march, the frame of errest.hip's k_err_march: block = 256 lanes = 512
// columns, one column pair per lane (16-byte loads on the pitched arrays, which
// share arow0 and pitch), grid (strips, row groups), rows [r_first + g * R, ...)
// and all columns 0..n.  A pair at c0 <= n lies inside the pitch (pitch even and
// >= n + 1); its second entry is stored only where c0 + 1 <= n.  Plain loads:
// the next step reads all three arrays again.
template <int LV, int ST>
__global__ __launch_bounds__(256) void k_dense_march(const double *__restrict__ u,
                                                     const double *__restrict__ h,
                                                     const double *__restrict__ h2, long arow0,
                                                     long pitch, long n, long r_first, long r_end,
                                                     int rows_per_group, W wt,
                                                     double *__restrict__ out, long orow0) {
    const long c0 = (long)blockIdx.x * 512 + 2 * threadIdx.x;
    if (c0 > n) return;
    const bool has1 = c0 + 1 <= n;
    const long i0 = r_first + (long)blockIdx.y * rows_per_group;
    const long i1 = std::min<long>(r_end, i0 + rows_per_group);
    const long w = n + 1;
    long o = (i0 - arow0) * pitch + c0;
    double *q = out + (i0 - orow0) * w + c0;
    // four rows' loads in flight before the first is consumed (a short last
    // batch re-reads its last row and skips the copies)
    for (long i = i0; i < i1; i += 4) {
        double2 x[4], y[4], z[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long d = std::min<long>(k, i1 - 1 - i);
            x[k] = ld2(u + o + d * pitch);
            if (LV >= 2) y[k] = ld2(h + o + d * pitch);
            if (LV >= 3) z[k] = ld2(h2 + o + d * pitch);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i + k < i1) {
                double2 v;
                v.x = point<LV>(x[k].x, LV >= 2 ? y[k].x : 0.0, LV >= 3 ? z[k].x : 0.0, wt);
                v.y = point<LV>(x[k].y, LV >= 2 ? y[k].y : 0.0, LV >= 3 ? z[k].y : 0.0, wt);
                store_pair<ST>(q + k * w, v, has1);
            }
        }
        o += 4 * pitch;
        q += 4 * w;
    }
}

// out[(A - A0) * ld + B] = interpolant(A * stride, B * stride): diag.hip's
// k_gather with up to three sources
template <int LV>
__global__ __launch_bounds__(256) void k_dense_gather(const double *__restrict__ u,
                                                      const double *__restrict__ h,
                                                      const double *__restrict__ h2, long arow0,
                                                      long pitch, long stride, long A0, long A1,
                                                      long cols, W wt, double *__restrict__ out,
                                                      long ld) {
    const long B = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (B >= cols) return;
    for (long A = A0 + blockIdx.y; A < A1; A += gridDim.y) {
        const long o = (A * stride - arow0) * pitch + B * stride;
        out[(A - A0) * ld + B] =
            point<LV>(u[o], LV >= 2 ? h[o] : 0.0, LV >= 3 ? h2[o] : 0.0, wt);
    }
}

// One lane per point.  The indices are checked before anything is addressed: a
// bad one gives NaN and reads nothing.
template <int LV>
__global__ __launch_bounds__(256) void k_dense_points(const double *__restrict__ u,
                                                      const double *__restrict__ h,
                                                      const double *__restrict__ h2, long arow0,
                                                      long pitch, long n, long ra, long rb,
                                                      bool fill_unheld, long npts,
                                                      const long *__restrict__ pi,
                                                      const long *__restrict__ pj, W wt,
                                                      double *__restrict__ out) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= npts) return;
    const long i = pi[k], j = pj[k];
    const bool valid = i >= 0 && i <= n && j >= 0 && j <= n;
    if (valid && i >= ra && i < rb) {
        const long o = (i - arow0) * pitch + j;
        out[k] = point<LV>(u[o], LV >= 2 ? h[o] : 0.0, LV >= 3 ? h2[o] : 0.0, wt);
    } else if (!valid || fill_unheld) {
        out[k] = __builtin_nan("");
    }
}

// Reference layout: one lane per point, grid-striding over (n+1)^2
template <int LV>
__global__ __launch_bounds__(256) void k_dense_raw(double *__restrict__ out,
                                                   const double *__restrict__ u,
                                                   const double *__restrict__ h,
                                                   const double *__restrict__ h2, long total,
                                                   W wt) {
    const long step = (long)gridDim.x * blockDim.x;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += step)
        out[q] = point<LV>(u[q], LV >= 2 ? h[q] : 0.0, LV >= 3 ? h2[q] : 0.0, wt);
}

// errest.hip's err_grid: about 4096 workgroups, >= 8 rows each; group_rows > 0
// (tuning key "dense_rows") sets the rows of a workgroup instead
void march_grid(long n, long rows, int group_rows, dim3 &g, int &R) {
    const unsigned strips = cdiv(n + 1, 512);
    const long want = std::max<long>(1, 4096 / (long)strips);
    R = (int)std::max<long>(8, (rows + want - 1) / want);
    if (group_rows > 0) R = (int)std::max<long>(group_rows, (rows + 65534) / 65535);
    g = dim3(strips, cdiv(rows, R));
}

thread_local double t_us = 0.0, t_bytes = 0.0;

}  // namespace

#define MGX_DENSE_BY_LEVELS(lv, CALL) \
    do {                              \
        if ((lv) == 1) {              \
            CALL(1);                  \
        } else if ((lv) == 2) {       \
            CALL(2);                  \
        } else {                      \
            CALL(3);                  \
        }                             \
    } while (0)

void launch_march(const Src &s, long r0, long r1, double *out, long orow0, int store,
                  int group_rows, hipStream_t st) {
    if (r1 <= r0) return;
    dim3 g;
    int R;
    march_grid(s.n, r1 - r0, group_rows, g, R);
    const W wt{s.w0, s.w1, s.w2};
#define ARGS s.u, s.h, s.h2, s.row0, s.pitch, s.n, r0, r1, R, wt, out, orow0
#define CALL(LV)                                                             \
    if (store == 1)                                                          \
        MGX_LAUNCH((k_dense_march<LV, 1>), g, dim3(256), st, ARGS);          \
    else if (store == 2)                                                     \
        MGX_LAUNCH((k_dense_march<LV, 2>), g, dim3(256), st, ARGS);          \
    else                                                                     \
        MGX_LAUNCH((k_dense_march<LV, 0>), g, dim3(256), st, ARGS)
    MGX_DENSE_BY_LEVELS(s.levels, CALL);
#undef CALL
#undef ARGS
}

void launch_gather(const Src &s, long stride, long A0, long A1, double *out, long ld,
                   hipStream_t st) {
    if (A1 <= A0) return;
    const long cols = s.n / stride + 1;
    const unsigned gy = (unsigned)std::min<long>(A1 - A0, 32768);
    const W wt{s.w0, s.w1, s.w2};
#define CALL(LV)                                                                                \
    MGX_LAUNCH(k_dense_gather<LV>, dim3(cdiv(cols, 256), gy), dim3(256), st, s.u, s.h, s.h2,    \
               s.row0, s.pitch, stride, A0, A1, cols, wt, out, ld)
    MGX_DENSE_BY_LEVELS(s.levels, CALL);
#undef CALL
}

void launch_points(const Src &s, long ra, long rb, bool fill_unheld, long npts, const long *pi,
                   const long *pj, double *out, hipStream_t st) {
    if (npts <= 0) return;
    const W wt{s.w0, s.w1, s.w2};
#define CALL(LV)                                                                               \
    MGX_LAUNCH(k_dense_points<LV>, dim3(cdiv(npts, 256)), dim3(256), st, s.u, s.h, s.h2,       \
               s.row0, s.pitch, s.n, ra, rb, fill_unheld, npts, pi, pj, wt, out)
    MGX_DENSE_BY_LEVELS(s.levels, CALL);
#undef CALL
}

void launch_raw(double *out, const double *u, const double *h, const double *h2, long n, double w0,
                double w1, double w2, int levels, hipStream_t st) {
    const long total = (n + 1) * (n + 1);
    const unsigned gx = (unsigned)std::min<long>((total + 255) / 256, 1L << 20);
    const W wt{w0, w1, w2};
#define CALL(LV) \
    MGX_LAUNCH(k_dense_raw<LV>, dim3(gx), dim3(256), st, out, u, h, h2, total, wt)
    MGX_DENSE_BY_LEVELS(levels, CALL);
#undef CALL
}

// ---------------------------------------------------------------- host
void PassTimer::begin(hipStream_t s) {
    if (hipEventCreate(&e0) != hipSuccess) e0 = nullptr;
    if (hipEventCreate(&e1) != hipSuccess) e1 = nullptr;
    if (e0) (void)hipEventRecord(e0, s);
}
void PassTimer::end(hipStream_t s) {
    if (e1) (void)hipEventRecord(e1, s);
}
void PassTimer::commit(double bytes) {
    float ms = 0.f;
    if (e0 && e1 && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) t_us += (double)ms * 1e3;
    t_bytes += bytes;
}
PassTimer::~PassTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
}
void timer_reset() { t_us = t_bytes = 0.0; }
void last_pass(double *us, double *bytes) {
    *us = t_us;
    *bytes = t_bytes;
}

}  // namespace mgxdense

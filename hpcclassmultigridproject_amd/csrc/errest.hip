// errest.hip -- the step error estimate on a two-deep history (errest.h).
//
// Built with -ffp-contract=off like every other translation unit: each product,
// difference and sum of the five formulas is rounded, the sums add the ROUNDED
// squares fl(x * x), and e = d / sc is the IEEE division.
#include "errest.h"

#include "stencil.h"

#include <algorithm>
#include <cmath>

namespace mgxerr {

using namespace mgx;
using mgxdiag::kMaxPartials;
using mgxdiag::kNoIdx;

namespace {

// ---------------------------------------------------------------- accumulator
// One lane's (wave's, workgroup's) running record.  The maxima compare by
// value; for |e| the smaller linear index wins among equal values, so that
// merging in any grouping gives the first occurrence in row-major order.
struct Acc {
    long nonfinite;
    double e_sq, e_mx;
    long e_idx;
    double d_sq, d_mx, c_sq, c_mx;
};

__device__ __forceinline__ Acc acc_zero() {
    Acc a;
    a.nonfinite = 0;
    a.e_sq = a.d_sq = a.c_sq = 0.0;
    a.e_mx = a.d_mx = a.c_mx = -__builtin_huge_val();
    a.e_idx = kNoIdx;
    return a;
}

struct Par {
    double p, w, atol, rtol;
};

// a lane visits its points in increasing linear index: the strict comparison
// keeps the first occurrence
__device__ __forceinline__ void acc_point(Acc &a, double u, double h, double h2, const Par &k,
                                          long idx) {
    const double ph = k.p * h;
    const double wh = k.w * h2;
    const double up = ph - wh;
    const double d = u - up;
    const double c = u - h;
    const double rs = k.rtol * fmax(fabs(u), fabs(h));
    const double sc = k.atol + rs;
    const double e = d / sc;
    const double ae = fabs(e);
    if (ae < __builtin_huge_val()) {   // finite (false for NaN and +-Inf)
        const double ad = fabs(d), ac = fabs(c);
        const double e2 = e * e;
        const double d2 = d * d;
        const double c2 = c * c;
        a.e_sq += e2;
        a.d_sq += d2;
        a.c_sq += c2;
        if (ae > a.e_mx) {
            a.e_mx = ae;
            a.e_idx = idx;
        }
        if (ad > a.d_mx) a.d_mx = ad;
        if (ac > a.c_mx) a.c_mx = ac;
    } else {
        a.nonfinite += 1;
    }
}

__device__ __forceinline__ void acc_merge(Acc &a, const Acc &b) {
    a.nonfinite += b.nonfinite;
    a.e_sq += b.e_sq;
    a.d_sq += b.d_sq;
    a.c_sq += b.c_sq;
    if (b.e_mx > a.e_mx || (b.e_mx == a.e_mx && b.e_idx < a.e_idx)) {
        a.e_mx = b.e_mx;
        a.e_idx = b.e_idx;
    }
    if (b.d_mx > a.d_mx) a.d_mx = b.d_mx;
    if (b.c_mx > a.c_mx) a.c_mx = b.c_mx;
}

// Wave butterfly (fixed order; every operation is symmetric in its operands,
// so all 64 lanes end with the same record), then the waves of the workgroup
// in wave order through LDS.  The result is valid in thread 0.
__device__ __forceinline__ Acc block_reduce(Acc a, Acc *lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Acc b;
        b.nonfinite = __shfl_xor(a.nonfinite, off, 64);
        b.e_sq = __shfl_xor(a.e_sq, off, 64);
        b.e_mx = __shfl_xor(a.e_mx, off, 64);
        b.e_idx = __shfl_xor(a.e_idx, off, 64);
        b.d_sq = __shfl_xor(a.d_sq, off, 64);
        b.d_mx = __shfl_xor(a.d_mx, off, 64);
        b.c_sq = __shfl_xor(a.c_sq, off, 64);
        b.c_mx = __shfl_xor(a.c_mx, off, 64);
        acc_merge(a, b);
    }
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) lds[w] = a;
    __syncthreads();
    Acc tot = acc_zero();
    if (threadIdx.x == 0) {
        const int nw = blockDim.x >> 6;
        for (int i = 0; i < nw; ++i) acc_merge(tot, lds[i]);
    }
    return tot;
}

__device__ __forceinline__ void store_rec(Rec *r, const Acc &a) {
    r->nonfinite = a.nonfinite;
    r->e_sq = a.e_sq;
    r->e_mx = a.e_mx;
    r->e_idx = a.e_idx;
    r->d_sq = a.d_sq;
    r->d_mx = a.d_mx;
    r->c_sq = a.c_sq;
    r->c_mx = a.c_mx;
}

// ---------------------------------------------------------------- kernels
// Row march, the frame of diag.hip's k_stats_march: block = 256 lanes = 512
// columns, one column pair per lane (16-byte loads on the three pitched
// arrays, which share row0 and pitch), grid (strips, row groups), interior rows
// [r_first + g * R, ...).  Plain loads: the next step reads all three again.
// Columns 0 and n and the pad columns up to the pitch take no part.  arow0 is
// the arrays' row origin: element (i, j) at a[(i - arow0) * pitch + j].
__global__ __launch_bounds__(256) void k_err_march(const double *__restrict__ u,
                                                   const double *__restrict__ h,
                                                   const double *__restrict__ h2, long arow0,
                                                   long pitch, long n, long r_first, long r_end,
                                                   int rows_per_group, Par par,
                                                   Rec *__restrict__ partials) {
    __shared__ Acc lds[4];
    const int t = threadIdx.x;
    const long c0 = (long)blockIdx.x * 512 + 2 * t;
    const bool use0 = c0 >= 1 && c0 <= n - 1, use1 = c0 + 1 <= n - 1;
    const long i0 = r_first + (long)blockIdx.y * rows_per_group;
    const long i1 = std::min<long>(r_end, i0 + rows_per_group);
    const long w = n + 1;
    Acc acc = acc_zero();
    if (use0 || use1) {   // c0 <= n - 1: the pair lies inside the pitch
        long o = (i0 - arow0) * pitch + c0;
        long idx = i0 * w + c0;
        // four rows' loads in flight before the first is consumed (a short
        // last batch re-reads its last row and skips the copies)
        for (long i = i0; i < i1; i += 4) {
            double2 x[4], y[4], z[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long d = std::min<long>(k, i1 - 1 - i);
                x[k] = ld2(u + o + d * pitch);
                y[k] = ld2(h + o + d * pitch);
                z[k] = ld2(h2 + o + d * pitch);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i + k < i1) {
                    if (use0) acc_point(acc, x[k].x, y[k].x, z[k].x, par, idx + k * w);
                    if (use1) acc_point(acc, x[k].y, y[k].y, z[k].y, par, idx + k * w + 1);
                }
            }
            o += 4 * pitch;
            idx += 4 * w;
        }
    }
    const Acc tot = block_reduce(acc, lds);
    if (t == 0) store_rec(partials + (long)blockIdx.y * gridDim.x + blockIdx.x, tot);
}

// Reference layout, one lane per point, the frame of diag.hip's k_stats_raw:
// the rows grid-stride over a capped gridDim.y.
__global__ __launch_bounds__(256) void k_err_raw(const double *__restrict__ u,
                                                 const double *__restrict__ h,
                                                 const double *__restrict__ h2, long n, Par par,
                                                 Rec *__restrict__ partials) {
    __shared__ Acc lds[4];
    const long w = n + 1;
    const long j = 1 + (long)blockIdx.x * blockDim.x + threadIdx.x;
    Acc acc = acc_zero();
    if (j <= n - 1) {
        for (long i = 1 + blockIdx.y; i < n; i += gridDim.y) {
            const long q = i * w + j;
            acc_point(acc, u[q], h[q], h2[q], par, q);
        }
    }
    const Acc tot = block_reduce(acc, lds);
    if (threadIdx.x == 0) store_rec(partials + (long)blockIdx.y * gridDim.x + blockIdx.x, tot);
}

// One workgroup: lane t takes partials t, t + 256, ... in index order, then
// the workgroup's reduction.  count == 0 gives the empty record.
__global__ __launch_bounds__(256) void k_err_final(const Rec *__restrict__ partials, int count,
                                                   Rec *__restrict__ out) {
    __shared__ Acc lds[4];
    Acc acc = acc_zero();
    for (int k = threadIdx.x; k < count; k += 256) {
        const Rec r = partials[k];
        Acc b;
        b.nonfinite = r.nonfinite;
        b.e_sq = r.e_sq;
        b.e_mx = r.e_mx;
        b.e_idx = r.e_idx;
        b.d_sq = r.d_sq;
        b.d_mx = r.d_mx;
        b.c_sq = r.c_sq;
        b.c_mx = r.c_mx;
        acc_merge(acc, b);
    }
    const Acc tot = block_reduce(acc, lds);
    if (threadIdx.x == 0) store_rec(out, tot);
}

// diag.hip's stats_grid: about 4096 workgroups, >= 8 rows each (strips *
// groups <= 4096 <= kMaxPartials while strips <= 4096)
void err_grid(long n, long rows, dim3 &g, int &R) {
    const unsigned strips = cdiv(n + 1, 512);
    rows = std::max<long>(rows, 1);
    const long want = std::max<long>(1, 4096 / (long)strips);
    R = (int)std::max<long>(8, (rows + want - 1) / want);
    g = dim3(strips, cdiv(rows, R));
}

thread_local double t_us = 0.0, t_bytes = 0.0;

}  // namespace

bool launch_step_error(const Args &a, hipStream_t s) {
    const long rows = a.r1 - a.r0;
    int count = 0;
    if (rows > 0 && a.n >= 2) {
        dim3 g;
        int R;
        err_grid(a.n, rows, g, R);
        if ((long)g.x * g.y > kMaxPartials) return false;
        count = (int)(g.x * g.y);
        const Par par{a.p, a.w, a.atol, a.rtol};
        MGX_LAUNCH(k_err_march, g, dim3(256), s, a.u, a.h, a.h2, a.row0, a.pitch, a.n, a.r0, a.r1,
                   R, par, a.partials);
    }
    MGX_LAUNCH(k_err_final, dim3(1), dim3(256), s, a.partials, count, a.out);
    return true;
}

bool launch_raw_step_error(const double *u, const double *h, const double *h2, long n, double p,
                           double w, double atol, double rtol, Rec *partials, Rec *out,
                           hipStream_t s) {
    int count = 0;
    if (n >= 2) {
        const long rows = n - 1, cols = n - 1;
        const long gx = cdiv(cols, 256);
        if (gx > kMaxPartials) return false;
        const long gy = std::max<long>(1, std::min<long>(rows, kMaxPartials / gx));
        count = (int)(gx * gy);
        const Par par{p, w, atol, rtol};
        MGX_LAUNCH(k_err_raw, dim3((unsigned)gx, (unsigned)gy), dim3(256), s, u, h, h2, n, par,
                   partials);
    }
    MGX_LAUNCH(k_err_final, dim3(1), dim3(256), s, partials, count, out);
    return true;
}

// ---------------------------------------------------------------- host
void to_step_err(const Rec &r, long n, long r0, long r1, double w, mgx_step_err *out) {
    const long rows = std::max<long>(0, r1 - r0), cols = std::max<long>(0, n - 1);
    out->count = rows * cols;
    out->nonfinite = r.nonfinite;
    out->w = w;
    out->err_sum_sq = r.e_sq;
    out->err_max = r.e_mx;
    const bool has = r.e_idx != kNoIdx;
    out->err_max_i = has ? r.e_idx / (n + 1) : -1;
    out->err_max_j = has ? r.e_idx % (n + 1) : -1;
    out->d_sum_sq = r.d_sq;
    out->d_max = r.d_mx;
    out->c_sum_sq = r.c_sq;
    out->c_max = r.c_mx;
}

bool merge(mgx_step_err *into, const mgx_step_err &o) {
    if (!(into->w == o.w)) return false;
    into->count += o.count;
    into->nonfinite += o.nonfinite;
    into->err_sum_sq += o.err_sum_sq;
    into->d_sum_sq += o.d_sum_sq;
    into->c_sum_sq += o.c_sum_sq;
    // (row, column) pairs order as the row-major position does, whatever n is
    auto before = [](long i, long j, long i2, long j2) { return i < i2 || (i == i2 && j < j2); };
    if (o.err_max_i >= 0 &&
        (into->err_max_i < 0 || o.err_max > into->err_max ||
         (o.err_max == into->err_max &&
          before(o.err_max_i, o.err_max_j, into->err_max_i, into->err_max_j)))) {
        into->err_max = o.err_max;
        into->err_max_i = o.err_max_i;
        into->err_max_j = o.err_max_j;
    }
    // (a record without a finite point carries -Inf here)
    if (o.d_max > into->d_max) into->d_max = o.d_max;
    if (o.c_max > into->c_max) into->c_max = o.c_max;
    return true;
}

bool tolerances_ok(double atol, double rtol) {
    return std::isfinite(atol) && std::isfinite(rtol) && atol >= 0 && rtol >= 0 &&
           (atol > 0 || rtol > 0);
}

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

}  // namespace mgxerr

// diag.hip -- field statistics and strided sampling on the device (diag.h).
//
// Built with -ffp-contract=off like every other translation unit: sum_sq adds
// the ROUNDED squares fl(x * x), and with `minus` every statistic is that of
// d = fl(a - minus), the bits numpy's a - w holds.
#include "diag.h"

#include "stencil.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace mgxdiag {

using namespace mgx;

namespace {

// ---------------------------------------------------------------- accumulator
// One lane's (wave's, workgroup's) running record.  Extrema compare by value;
// among equal values the smaller linear index wins, so that merging in any
// grouping gives the first occurrence in row-major order.
struct Acc {
    double sum, sum_abs, sum_sq;
    long nonfinite;
    double mn, mx;
    long mn_idx, mx_idx;
};

__device__ __forceinline__ Acc acc_zero() {
    Acc a;
    a.sum = a.sum_abs = a.sum_sq = 0.0;
    a.nonfinite = 0;
    a.mn = __builtin_huge_val();
    a.mx = -__builtin_huge_val();
    a.mn_idx = a.mx_idx = kNoIdx;
    return a;
}

// a lane visits its points in increasing linear index: strict comparisons keep
// the first occurrence
__device__ __forceinline__ void acc_point(Acc &a, double x, long idx) {
    const double ax = fabs(x);
    if (ax < __builtin_huge_val()) {   // finite (false for NaN and +-Inf)
        a.sum += x;
        a.sum_abs += ax;
        const double sq = x * x;
        a.sum_sq += sq;
        if (x < a.mn) {
            a.mn = x;
            a.mn_idx = idx;
        }
        if (x > a.mx) {
            a.mx = x;
            a.mx_idx = idx;
        }
    } else {
        a.nonfinite += 1;
    }
}

__device__ __forceinline__ void acc_merge(Acc &a, const Acc &b) {
    a.sum += b.sum;
    a.sum_abs += b.sum_abs;
    a.sum_sq += b.sum_sq;
    a.nonfinite += b.nonfinite;
    if (b.mn < a.mn || (b.mn == a.mn && b.mn_idx < a.mn_idx)) {
        a.mn = b.mn;
        a.mn_idx = b.mn_idx;
    }
    if (b.mx > a.mx || (b.mx == a.mx && b.mx_idx < a.mx_idx)) {
        a.mx = b.mx;
        a.mx_idx = b.mx_idx;
    }
}

// Wave butterfly (fixed order; every operation is symmetric in its operands,
// so all 64 lanes end with the same record), then the waves of the workgroup
// in wave order through LDS.  The result is valid in thread 0.
__device__ __forceinline__ Acc block_reduce(Acc a, Acc *lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Acc b;
        b.sum = __shfl_xor(a.sum, off, 64);
        b.sum_abs = __shfl_xor(a.sum_abs, off, 64);
        b.sum_sq = __shfl_xor(a.sum_sq, off, 64);
        b.nonfinite = __shfl_xor(a.nonfinite, off, 64);
        b.mn = __shfl_xor(a.mn, off, 64);
        b.mx = __shfl_xor(a.mx, off, 64);
        b.mn_idx = __shfl_xor(a.mn_idx, off, 64);
        b.mx_idx = __shfl_xor(a.mx_idx, off, 64);
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
    r->sum = a.sum;
    r->sum_abs = a.sum_abs;
    r->sum_sq = a.sum_sq;
    r->mn = a.mn;
    r->mx = a.mx;
    r->mn_idx = a.mn_idx;
    r->mx_idx = a.mx_idx;
}

// ---------------------------------------------------------------- kernels
// Row march, the frame of source.hip's k_rhs_source: block = 256 lanes = 512
// columns, one column pair per lane (16-byte loads on the pitched array), grid
// (strips, row groups), rows [r_first + g * R, ...).  Plain loads: the next
// step reads the field again.  Columns outside [j0, j1] -- the pad columns up
// to the pitch among them, which hold zeros -- take no part.  MINUS: the
// statistics of fl(a - m), m in the reference layout (rows 8-byte aligned:
// 8-byte loads).
template <bool MINUS>
__global__ __launch_bounds__(256) void k_stats_march(
    const double *__restrict__ a, long arow0, long pitch, const double *__restrict__ m,
    long mrow0, long n, long r_first, long r_end, long j0, long j1, int rows_per_group,
    Rec *__restrict__ partials) {
    __shared__ Acc lds[4];
    const int t = threadIdx.x;
    const long c0 = (long)blockIdx.x * 512 + 2 * t;
    const bool use0 = c0 >= j0 && c0 <= j1, use1 = c0 + 1 >= j0 && c0 + 1 <= j1;
    const long i0 = r_first + (long)blockIdx.y * rows_per_group;
    const long i1 = std::min<long>(r_end, i0 + rows_per_group);
    const long w = n + 1;
    Acc acc = acc_zero();
    if (use0 || use1) {   // c0 <= j1 <= n: the pair lies inside the pitch
        const double *row = a + (i0 - arow0) * pitch + c0;
        const double *mr = MINUS ? m + (i0 - mrow0) * w + c0 : nullptr;
        long idx = i0 * w + c0;
        // four rows' loads in flight before the first is consumed (a short
        // last batch re-reads its last row and skips the copies)
        for (long i = i0; i < i1; i += 4) {
            double2 x[4];
            double m0[4], m1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long d = std::min<long>(k, i1 - 1 - i);
                x[k] = ld2(row + d * pitch);
                if (MINUS) {
                    m0[k] = use0 ? mr[d * w] : 0.0;
                    m1[k] = use1 ? mr[d * w + 1] : 0.0;   // c0 + 1 <= n
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i + k < i1) {
                    double2 v = x[k];
                    if (MINUS) {
                        v.x = v.x - m0[k];
                        v.y = v.y - m1[k];
                    }
                    if (use0) acc_point(acc, v.x, idx + k * w);
                    if (use1) acc_point(acc, v.y, idx + k * w + 1);
                }
            }
            row += 4 * pitch;
            if (MINUS) mr += 4 * w;
            idx += 4 * w;
        }
    }
    const Acc tot = block_reduce(acc, lds);
    if (t == 0) store_rec(partials + (long)blockIdx.y * gridDim.x + blockIdx.x, tot);
}

// Reference layout, one lane per point, the frame of source.hip's
// k_raw_rhs_source: the rows grid-stride over a capped gridDim.y.
template <bool MINUS>
__global__ __launch_bounds__(256) void k_stats_raw(const double *__restrict__ a,
                                                   const double *__restrict__ m, long n,
                                                   long r0, long r1, long j0, long j1,
                                                   Rec *__restrict__ partials) {
    __shared__ Acc lds[4];
    const long w = n + 1;
    const long j = j0 + (long)blockIdx.x * blockDim.x + threadIdx.x;
    Acc acc = acc_zero();
    if (j <= j1) {
        for (long i = r0 + blockIdx.y; i < r1; i += gridDim.y) {
            const long p = i * w + j;
            double x = a[p];
            if (MINUS) x = x - m[p];
            acc_point(acc, x, p);
        }
    }
    const Acc tot = block_reduce(acc, lds);
    if (threadIdx.x == 0) store_rec(partials + (long)blockIdx.y * gridDim.x + blockIdx.x, tot);
}

// One workgroup: lane t takes partials t, t + 256, ... in index order, then
// the workgroup's reduction.  count == 0 gives the empty record.
__global__ __launch_bounds__(256) void k_stats_final(const Rec *__restrict__ partials, int count,
                                                     Rec *__restrict__ out) {
    __shared__ Acc lds[4];
    Acc acc = acc_zero();
    for (int k = threadIdx.x; k < count; k += 256) {
        const Rec r = partials[k];
        Acc b;
        b.sum = r.sum;
        b.sum_abs = r.sum_abs;
        b.sum_sq = r.sum_sq;
        b.nonfinite = r.nonfinite;
        b.mn = r.mn;
        b.mx = r.mx;
        b.mn_idx = r.mn_idx;
        b.mx_idx = r.mx_idx;
        acc_merge(acc, b);
    }
    const Acc tot = block_reduce(acc, lds);
    if (threadIdx.x == 0) store_rec(out, tot);
}

// out[(A - A0) * ld + B] = a(A * stride, B * stride): one lane per sampled
// column, the sampled rows grid-striding
__global__ __launch_bounds__(256) void k_gather(const double *__restrict__ a, long arow0,
                                                long pitch, long stride, long A0, long A1,
                                                long cols, double *__restrict__ out, long ld) {
    const long B = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (B >= cols) return;
    for (long A = A0 + blockIdx.y; A < A1; A += gridDim.y)
        out[(A - A0) * ld + B] = a[(A * stride - arow0) * pitch + B * stride];
}

// the row cut of kernels.hip's res_grid: about 4096 workgroups, >= 8 rows each
// (strips * groups <= 4096 <= kMaxPartials while strips <= 4096)
void stats_grid(long n, long rows, dim3 &g, int &R) {
    const unsigned strips = cdiv(n + 1, 512);
    rows = std::max<long>(rows, 1);
    const long want = std::max<long>(1, 4096 / (long)strips);
    R = (int)std::max<long>(8, (rows + want - 1) / want);
    g = dim3(strips, cdiv(rows, R));
}

thread_local double t_us = 0.0, t_bytes = 0.0;

}  // namespace

void launch_stats(const StatsArgs &a, hipStream_t s) {
    const long rows = a.r1 - a.r0;
    int count = 0;
    if (rows > 0 && a.j1 >= a.j0) {
        dim3 g;
        int R;
        stats_grid(a.f.n, rows, g, R);
        if ((long)g.x * g.y <= kMaxPartials) {
            count = (int)(g.x * g.y);
            if (a.minus)
                MGX_LAUNCH(k_stats_march<true>, g, dim3(256), s, a.f.a, a.f.row0, a.f.pitch, a.minus,
                           a.minus_row0, a.f.n, a.r0, a.r1, a.j0, a.j1, R, a.partials);
            else
                MGX_LAUNCH(k_stats_march<false>, g, dim3(256), s, a.f.a, a.f.row0, a.f.pitch,
                           (const double *)nullptr, 0L, a.f.n, a.r0, a.r1, a.j0, a.j1, R,
                           a.partials);
        }
    }
    MGX_LAUNCH(k_stats_final, dim3(1), dim3(256), s, a.partials, count, a.out);
}

bool launch_raw_stats(const double *a, const double *minus, long n, long r0, long r1, long j0,
                      long j1, Rec *partials, Rec *out, hipStream_t s) {
    const long rows = r1 - r0, cols = j1 - j0 + 1;
    int count = 0;
    if (rows > 0 && cols > 0) {
        const long gx = cdiv(cols, 256);
        if (gx > kMaxPartials) return false;
        const long gy = std::max<long>(1, std::min<long>(rows, kMaxPartials / gx));
        count = (int)(gx * gy);
        const dim3 g((unsigned)gx, (unsigned)gy);
        if (minus)
            MGX_LAUNCH(k_stats_raw<true>, g, dim3(256), s, a, minus, n, r0, r1, j0, j1, partials);
        else
            MGX_LAUNCH(k_stats_raw<false>, g, dim3(256), s, a, (const double *)nullptr, n, r0, r1,
                       j0, j1, partials);
    }
    MGX_LAUNCH(k_stats_final, dim3(1), dim3(256), s, partials, count, out);
    return true;
}

void launch_gather(const View &f, long stride, long A0, long A1, double *out, long ld,
                   hipStream_t s) {
    if (A1 <= A0) return;
    const long cols = f.n / stride + 1;
    const unsigned gy = (unsigned)std::min<long>(A1 - A0, 32768);
    MGX_LAUNCH(k_gather, dim3(cdiv(cols, 256), gy), dim3(256), s, f.a, f.row0, f.pitch, stride, A0,
               A1, cols, out, ld);
}

// ---------------------------------------------------------------- host
void to_stats(const Rec &r, long n, long r0, long r1, long j0, long j1, mgx_stats *out) {
    const long rows = std::max<long>(0, r1 - r0), cols = std::max<long>(0, j1 - j0 + 1);
    out->count = rows * cols;
    out->nonfinite = r.nonfinite;
    out->sum = r.sum;
    out->sum_abs = r.sum_abs;
    out->sum_sq = r.sum_sq;
    out->min = r.mn;
    out->max = r.mx;
    const long w = n + 1;
    const bool hmn = r.mn_idx != kNoIdx, hmx = r.mx_idx != kNoIdx;
    out->min_i = hmn ? r.mn_idx / w : -1;
    out->min_j = hmn ? r.mn_idx % w : -1;
    out->max_i = hmx ? r.mx_idx / w : -1;
    out->max_j = hmx ? r.mx_idx % w : -1;
}

void merge(mgx_stats *into, const mgx_stats &o) {
    into->count += o.count;
    into->nonfinite += o.nonfinite;
    into->sum += o.sum;
    into->sum_abs += o.sum_abs;
    into->sum_sq += o.sum_sq;
    // (row, column) pairs order as the row-major position does, whatever n is
    auto before = [](long i, long j, long i2, long j2) { return i < i2 || (i == i2 && j < j2); };
    if (o.min_i >= 0 &&
        (into->min_i < 0 || o.min < into->min ||
         (o.min == into->min && before(o.min_i, o.min_j, into->min_i, into->min_j)))) {
        into->min = o.min;
        into->min_i = o.min_i;
        into->min_j = o.min_j;
    }
    if (o.max_i >= 0 &&
        (into->max_i < 0 || o.max > into->max ||
         (o.max == into->max && before(o.max_i, o.max_j, into->max_i, into->max_j)))) {
        into->max = o.max;
        into->max_i = o.max_i;
        into->max_j = o.max_j;
    }
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

}  // namespace mgxdiag

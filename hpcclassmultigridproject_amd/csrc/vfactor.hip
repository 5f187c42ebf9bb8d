// vfactor.hip -- device backend of the exact rank-1 velocity factorisation
// (vfactor.h; the decisions are sepvel.h's factor_rank1_on, shared with the
// host backend).
#include "vfactor.h"

#include <algorithm>
#include <cfloat>
#include <vector>

#include "sepvel.h"

namespace mgxvf {

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 32;        // rows one workgroup marches per work item
constexpr int kMaxBlocks = 2048; // memory-bound: cap the grid, stride the rest

thread_local int t_rounds = 0;
thread_local double t_ms = -1.0;

// out[i] = v[i][js]
__global__ __launch_bounds__(kThreads) void k_vf_column(const double *__restrict__ v, long rows,
                                                       long ld, long js,
                                                       double *__restrict__ out) {
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < rows;
         i += (long)gridDim.x * kThreads)
        out[i] = v[i * ld + js];
}

// One work item = kRows rows x (kThreads * V) columns: each lane keeps the
// column factors of its V adjacent columns in registers and marches down the
// rows (a[i] is wave-uniform), so a row of the item is one contiguous
// kThreads * V * 8 byte read.  bad[j] = 1 where a product's bits differ from
// the stored entry's (signed zeros, NaN and Inf compare as bits); *range_bad =
// 1 where a nonzero |v| * smin is subnormal.  Plain stores of the same value:
// no atomics.  V = 2 needs v 16-byte aligned and ld even.
template <int V>
__global__ __launch_bounds__(kThreads) void k_vf_check(const double *__restrict__ v, long rows,
                                                      long w, long ld,
                                                      const double *__restrict__ a,
                                                      const double *__restrict__ b, double smin,
                                                      int *__restrict__ bad,
                                                      int *__restrict__ range_bad, long ctiles,
                                                      long items) {
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long ct = it % ctiles, r0 = (it / ctiles) * kRows;
        const long r1 = r0 + kRows < rows ? r0 + kRows : rows;
        const long j = (ct * kThreads + threadIdx.x) * V;
        if (j >= w) continue;
        // (the last column of an odd width has no partner: an 8-byte load, so
        // nothing past the row's w entries is read)
        const bool two = V == 2 && j + 1 < w;
        const double b0 = b[j], b1 = two ? b[j + 1] : 0.0;
        bool f0 = false, f1 = false, rg = false;
#pragma unroll 4
        for (long i = r0; i < r1; ++i) {
            const double ai = a[i];
            const double *p = v + i * ld + j;
            double x0, x1 = 0.0;
            if (two) {
                const double2 x = *reinterpret_cast<const double2 *>(p);
                x0 = x.x;
                x1 = x.y;
            } else {
                x0 = *p;
            }
            f0 |= __double_as_longlong(ai * b0) != __double_as_longlong(x0);
            rg |= x0 != 0.0 && fabs(x0) * smin < DBL_MIN;
            if (two) {
                f1 |= __double_as_longlong(ai * b1) != __double_as_longlong(x1);
                rg |= x1 != 0.0 && fabs(x1) * smin < DBL_MIN;
            }
        }
        if (f0) bad[j] = 1;
        if (f1) bad[j + 1] = 1;
        if (rg && smin > 0.0) *range_bad = 1;
    }
}

// sepvel.h backend (see HostField there) on a device-resident field.
struct DeviceField {
    const double *v;
    long rows, w, ld;
    double smin;
    hipStream_t s;
    double *da = nullptr, *db = nullptr;
    int *dflags = nullptr;   // w column flags + the range flag
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::vector<double> hrows;
    std::vector<int> hflags;
    hipError_t err = hipSuccess;
    bool range_bad = false;
    int rounds = 0;
    double ms = 0.0;

    bool ok(hipError_t e) {
        if (e != hipSuccess && err == hipSuccess) err = e;
        return err == hipSuccess;
    }
    bool init() {
        return ok(hipMalloc(&da, sizeof(double) * (size_t)rows)) &&
               ok(hipMalloc(&db, sizeof(double) * (size_t)w)) &&
               ok(hipMalloc(&dflags, sizeof(int) * (size_t)(w + 1))) && ok(hipEventCreate(&e0)) &&
               ok(hipEventCreate(&e1));
    }
    ~DeviceField() {
        (void)hipFree(da);
        (void)hipFree(db);
        (void)hipFree(dflags);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    // (the row factors stay in da for check(): the host logic does not change
    // them between column() and check())
    void column(long js, double *a) {
        std::fill(a, a + rows, 0.0);
        if (err != hipSuccess) return;
        const int grid = (int)std::min<long>((rows + kThreads - 1) / kThreads, kMaxBlocks);
        k_vf_column<<<grid, kThreads, 0, s>>>(v, rows, ld, js, da);
        if (ok(hipGetLastError()) &&
            ok(hipMemcpyAsync(a, da, sizeof(double) * (size_t)rows, hipMemcpyDeviceToHost, s)))
            ok(hipStreamSynchronize(s));
        if (err != hipSuccess) std::fill(a, a + rows, 0.0);
    }
    void pivot_rows(const long *piv, int np, const double **out) {
        hrows.assign((size_t)np * (size_t)w, 0.0);
        for (int k = 0; k < np; ++k) {
            out[k] = hrows.data() + (size_t)k * (size_t)w;
            if (err == hipSuccess)
                ok(hipMemcpyAsync(hrows.data() + (size_t)k * (size_t)w, v + piv[k] * ld,
                                  sizeof(double) * (size_t)w, hipMemcpyDeviceToHost, s));
        }
        if (err == hipSuccess) ok(hipStreamSynchronize(s));
    }
    long check(const double *, const double *b, unsigned char *bad, long) {
        if (err != hipSuccess) return -1;
        const bool vec = ((uintptr_t)v & 15) == 0 && (ld & 1) == 0;
        const long per = kThreads * (vec ? 2 : 1);
        const long ctiles = (w + per - 1) / per;
        const long items = ctiles * ((rows + kRows - 1) / kRows);
        const int grid = (int)std::min<long>(items, kMaxBlocks);
        hflags.assign((size_t)w + 1, 0);
        if (!ok(hipMemcpyAsync(db, b, sizeof(double) * (size_t)w, hipMemcpyHostToDevice, s)) ||
            !ok(hipMemsetAsync(dflags, 0, sizeof(int) * (size_t)(w + 1), s)) ||
            !ok(hipEventRecord(e0, s)))
            return -1;
        if (vec)
            k_vf_check<2><<<grid, kThreads, 0, s>>>(v, rows, w, ld, da, db, smin, dflags,
                                                    dflags + w, ctiles, items);
        else
            k_vf_check<1><<<grid, kThreads, 0, s>>>(v, rows, w, ld, da, db, smin, dflags,
                                                    dflags + w, ctiles, items);
        if (!ok(hipGetLastError()) || !ok(hipEventRecord(e1, s)) ||
            !ok(hipMemcpyAsync(hflags.data(), dflags, sizeof(int) * (size_t)(w + 1),
                               hipMemcpyDeviceToHost, s)) ||
            !ok(hipStreamSynchronize(s)))
            return -1;
        float t = 0.f;
        if (hipEventElapsedTime(&t, e0, e1) == hipSuccess) ms += t;
        ++rounds;
        long nbad = 0;
        for (long j = 0; j < w; ++j) {
            bad[j] = hflags[(size_t)j] ? 1 : 0;
            nbad += bad[j];
        }
        range_bad = hflags[(size_t)w] != 0;
        return nbad;
    }
    // the range flag of the last check(): the pass that found every entry equal
    bool range_ok(double) const { return !range_bad; }
};

}  // namespace

int factor_rank1_device(const double *v, long rows, long w, long ld, double smin, double *a,
                        double *b, hipStream_t stream, long *jsel, hipError_t *err) {
    t_rounds = 0;
    t_ms = -1.0;
    if (err) *err = hipSuccess;
    if (!v || !a || !b || rows < 1 || w < 1 || ld < w) return 0;
    DeviceField F{v, rows, w, ld, smin, stream};
    bool done = false;
    if (F.init()) done = mgxsep::factor_rank1_on(F, rows, w, smin, a, b, jsel);
    t_rounds = F.rounds;
    t_ms = F.ms;
    if (F.err != hipSuccess) {
        if (err) *err = F.err;
        return -1;
    }
    return done ? 1 : 0;
}

void last_stats(int *rounds, double *ms) {
    if (rounds) *rounds = t_rounds;
    if (ms) *ms = t_ms;
}

}  // namespace mgxvf

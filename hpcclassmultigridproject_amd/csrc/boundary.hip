// boundary.hip -- scatter and gather of the Dirichlet ring (boundary.h).
//
// The ring is 4(n+1) doubles against (n+1)^2 of the field: both kernels are
// launch-latency bound, so the only thing to get right is the access shape.
// Rows 0 and n are contiguous: one lane per column, 8-byte coalesced accesses
// (a side of g starts on an 8-byte boundary only, n+1 being odd).  Columns 0
// and n are one 8-byte access per row at a stride of the pitch -- every lane a
// cache line of its own.  The two shapes never share a wavefront: blockIdx.y
// selects the side (0: row 0, 1: row n, 2: both columns), so a workgroup is
// all coalesced or all strided.
#include "boundary.h"

#include "stencil.h"

#include <algorithm>

namespace mgxbc {

using namespace mgx;

namespace {

constexpr int kLanes = 256;

__global__ __launch_bounds__(kLanes) void k_ring_scatter(double *__restrict__ u, long pitch,
                                                         long n, long lo, long hi,
                                                         const double *__restrict__ g) {
    const long k = (long)blockIdx.x * kLanes + threadIdx.x;
    const long w = n + 1;
    if (blockIdx.y == 0) {   // row 0
        if (lo == 0 && k <= n) u[k] = g[k];
    } else if (blockIdx.y == 1) {   // row n
        if (hi == n && k <= n) u[(n - lo) * pitch + k] = g[w + k];
    } else {   // columns 0 and n of the held rows; the corners are the rows'
        const long i = lo + k;
        if (i <= hi && i > 0 && i < n) {
            double *row = u + k * pitch;
            row[0] = g[2 * w + i];
            row[n] = g[3 * w + i];
        }
    }
}

__global__ __launch_bounds__(kLanes) void k_ring_gather(const double *__restrict__ u, long pitch,
                                                        long n, long lo, long r0, long r1,
                                                        double *__restrict__ g) {
    const long k = (long)blockIdx.x * kLanes + threadIdx.x;
    const long w = n + 1;
    if (blockIdx.y == 0) {
        if (r0 == 0 && k <= n) g[k] = u[(0 - lo) * pitch + k];
    } else if (blockIdx.y == 1) {
        if (r1 == n && k <= n) g[w + k] = u[(n - lo) * pitch + k];
    } else {
        const long i = r0 + k;
        if (i <= r1) {
            const double *row = u + (i - lo) * pitch;
            g[2 * w + i] = row[0];
            g[3 * w + i] = row[n];
        }
    }
}

thread_local double t_us = 0.0;

}  // namespace

void launch_scatter(double *u, long pitch, long n, long lo, long hi, const double *g,
                    hipStream_t s) {
    if (hi < lo) return;
    const long span = std::max<long>(n + 1, hi - lo + 1);
    MGX_LAUNCH(k_ring_scatter, dim3(cdiv(span, kLanes), 3), dim3(kLanes), s, u, pitch, n, lo, hi, g);
}

void launch_gather(const double *u, long pitch, long n, long lo, long r0, long r1, double *g,
                   hipStream_t s) {
    if (r1 < r0) return;
    const long span = std::max<long>(n + 1, r1 - r0 + 1);
    MGX_LAUNCH(k_ring_gather, dim3(cdiv(span, kLanes), 3), dim3(kLanes), s, u, pitch, n, lo, r0, r1,
               g);
}

void RingTimer::begin(hipStream_t s) {
    if (!e0 && hipEventCreate(&e0) != hipSuccess) e0 = nullptr;
    if (!e1 && hipEventCreate(&e1) != hipSuccess) e1 = nullptr;
    if (e0) (void)hipEventRecord(e0, s);
}
void RingTimer::end(hipStream_t s) {
    if (e1) (void)hipEventRecord(e1, s);
}
void RingTimer::commit() {
    float ms = 0.f;
    if (e0 && e1 && hipEventSynchronize(e1) == hipSuccess &&
        hipEventElapsedTime(&ms, e0, e1) == hipSuccess)
        t_us = (double)ms * 1e3;
    else
        (void)hipGetLastError();
}
void RingTimer::destroy() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    e0 = e1 = nullptr;
}
double last_us() { return t_us; }

}  // namespace mgxbc

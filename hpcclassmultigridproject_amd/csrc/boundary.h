// boundary.h -- the Dirichlet ring of u written and read on the device
// (csrc/boundary.hip): mgx_set_boundary / mgx_get_boundary / mgx_write_boundary.
//
// The ring g of a level with n+1 rows and columns holds 4(n+1) doubles,
// side-major:
//     g[0*(n+1) + j] = u(0, j)      g[2*(n+1) + i] = u(i, 0)
//     g[1*(n+1) + j] = u(n, j)      g[3*(n+1) + i] = u(i, n)
// The four corners belong to the two row sides: the scatter never reads entries
// 0 and n of sides 2 and 3, the gather fills them with the corner values.
//
// Both kernels work on a pitched buffer that holds rows [lo, hi] of the level
// (a whole level: lo = 0, hi = n; a part of a partitioned context: its
// allocated rows, ghost rows included).  Plain vector stores, no atomics, no
// LDS: every ring entry has exactly one writer.
#pragma once
#include <hip/hip_runtime.h>

namespace mgxbc {

// entries of a ring
inline long ring_size(long n) { return 4 * (n + 1); }

// u: the buffer's first row (global row lo), rows [lo, hi], row pitch `pitch`
// (>= n+1; the reference layout has pitch n+1).  Rows 0 and n are written where
// the buffer holds them; columns 0 and n of every other held row.
void launch_scatter(double *u, long pitch, long n, long lo, long hi, const double *g,
                    hipStream_t s);
// The ring entries of rows [r0, r1] (lo <= r0, r1 <= the buffer's last row) of
// such a buffer into g: rows 0 and n where the range holds them, and entries
// r0..r1 of the two column sides (corners included).
void launch_gather(const double *u, long pitch, long n, long lo, long r0, long r1, double *g,
                   hipStream_t s);

// Device time of the calling thread's last ring write (tuning key
// "boundary_us"): HIP events around its launches, read once they have passed.
struct RingTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    void begin(hipStream_t s);   // creates the events on first use
    void end(hipStream_t s);
    void commit();               // waits for the end event
    void destroy();
};
double last_us();

}  // namespace mgxbc

// diag.h -- on-device field diagnostics (csrc/diag.hip): a one-pass statistics
// reduction and a strided gather, so that a run can watch a field (mass,
// extrema and where, norms, non-finite count, a coarse picture) without moving
// it to the host.
//
// One pass gives, over a row / column window of a field or of fl(a - minus):
//   nonfinite            NaN or +-Inf entries,
//   sum, sum_abs, sum_sq over the FINITE entries x: x, |x|, fl(x * x)
//                        (never contracted: -ffp-contract=off),
//   min, max             over the finite entries, by value (-0 == +0), the
//                        first occurrence in row-major order among equals,
//                        with that entry's bits and its linear index
//                        i * (n + 1) + j.
// Two stages, no atomics: every workgroup writes one partial record, a
// single-workgroup kernel combines them in index order.  The order of every
// addition is a fixed function of (n, row range, column range): two calls give
// the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mgx.h"

namespace mgxdiag {

// the device record (partials and result)
struct Rec {
    long nonfinite;
    double sum, sum_abs, sum_sq;
    double mn, mx;   // +Inf / -Inf when there is no finite entry
    long mn_idx, mx_idx;   // linear index i*(n+1)+j; kNoIdx when there is none
};
constexpr long kNoIdx = 0x7fffffffffffffffL;
// most partial records of one launch
constexpr int kMaxPartials = 8192;
// scratch of a caller: kMaxPartials partials followed by `nrec` result records
inline size_t scratch_bytes(int nrec) { return sizeof(Rec) * (size_t)(kMaxPartials + nrec); }

// A field: element (i, j) at a[(i - row0) * pitch + j], 0 <= j <= n.
struct View {
    const double *a = nullptr;
    long row0 = 0, pitch = 0, n = 0;
};

struct StatsArgs {
    View f;                 // tower layout: pitch % 2 == 0 and a 16-byte aligned
    const double *minus = nullptr;   // reference layout (pitch n+1), or null
    long minus_row0 = 0;    // minus holds rows from minus_row0 on
    long r0 = 0, r1 = 0;    // rows [r0, r1)
    long j0 = 0, j1 = 0;    // columns [j0, j1]
    Rec *partials = nullptr;   // kMaxPartials records
    Rec *out = nullptr;        // the result record
};
// Row march over a pitched field (256 lanes = 512 columns per workgroup, one
// column pair per lane with 16-byte loads, minus with 8-byte loads), then the
// final kernel.  An empty window launches the final kernel alone.
void launch_stats(const StatsArgs &a, hipStream_t s);
// Reference layout on both operands (rows only 8-byte aligned): one lane per
// point, the rows grid-striding.  Returns false when n is too large for the
// partial buffer (n + 1 > 256 * kMaxPartials).
bool launch_raw_stats(const double *a, const double *minus, long n, long r0, long r1, long j0,
                      long j1, Rec *partials, Rec *out, hipStream_t s);

// out[(A - A0) * ld + B] = f(A * stride, B * stride), A0 <= A < A1, 0 <= B <= n / stride
void launch_gather(const View &f, long stride, long A0, long A1, double *out, long ld,
                   hipStream_t s);

// Host: the public struct of a device record over rows [r0, r1) x columns [j0, j1]
void to_stats(const Rec &r, long n, long r0, long r1, long j0, long j1, mgx_stats *out);
// Host: mgx_stats_merge
void merge(mgx_stats *into, const mgx_stats &other);

// Device time of the calling thread's stats launches since timer_reset(), and
// their compulsory bytes (tuning keys "stats_us" / "stats_bytes").
struct PassTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    void begin(hipStream_t s);
    void end(hipStream_t s);
    void commit(double bytes);   // after the stream has been synchronised
    ~PassTimer();
};
void timer_reset();
void last_pass(double *us, double *bytes);

}  // namespace mgxdiag

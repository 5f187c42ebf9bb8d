// errest.h -- the step error estimate on a two-deep history (csrc/errest.hip).
//
// With the last three time levels resident -- u = u^(n+1), h = u^n, h2 =
// u^(n-1) (mgx_set_history_depth(ctx, 2)) -- one reduction pass gives the
// record mgx_step_err of include/mgx.h.  All C doubles, every operation
// rounded, nothing contracted (-ffp-contract=off), the division the true one;
// on the host w = dt_prev / dt_prev2 and p = 1.0 + w, and at every interior
// point
//     up = fl( fl(p * h) - fl(w * h2) )
//     d  = fl( u - up )
//     c  = fl( u - h )
//     sc = fl( atol + fl( rtol * max(|u|, |h|) ) )
//     e  = d / sc
// A point whose e is NaN or +-Inf counts in `nonfinite` and in nothing else.
// Over the others: the sums of fl(x * x) and the maxima of |x| for x = e, d, c,
// and for |e| the linear index i * (n + 1) + j of the first occurrence in
// row-major order.
// Two stages in the frame of diag.hip's statistics pass, no atomics: every
// workgroup writes one partial record, a single-workgroup kernel combines them
// in index order.  The order of every addition is a fixed function of (n, row
// range): two calls give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mgx.h"
#include "diag.h"

namespace mgxerr {

// the device record (partials and result); the size of a mgxdiag::Rec, so that
// a context's diagnostics scratch (mgxdiag::scratch_bytes) serves both passes
struct Rec {
    long nonfinite;
    double e_sq, e_mx;   // e_mx, d_mx, c_mx: -Inf when there is no finite point
    long e_idx;          // mgxdiag::kNoIdx when there is none
    double d_sq, d_mx, c_sq, c_mx;
};
static_assert(sizeof(Rec) == sizeof(mgxdiag::Rec), "the diagnostics scratch holds either record");

struct Args {
    // tower layout, all three alike: element (i, j) at a[(i - row0) * pitch + j],
    // pitch % 2 == 0 and the arrays 16-byte aligned
    const double *u = nullptr, *h = nullptr, *h2 = nullptr;
    long row0 = 0, pitch = 0, n = 0;
    long r0 = 0, r1 = 0;   // interior rows [r0, r1), 1 <= r0, r1 <= n
    double p = 0, w = 0, atol = 0, rtol = 0;
    Rec *partials = nullptr;   // mgxdiag::kMaxPartials records
    Rec *out = nullptr;        // the result record
};
// Row march (256 lanes = 512 columns per workgroup, one column pair per lane,
// 16-byte loads from u, h and h2), then the final kernel.  An empty row range
// launches the final kernel alone.  false: the level is too wide for the
// partial buffer (nothing launched).
bool launch_step_error(const Args &a, hipStream_t s);
// Reference layout (pitch n+1, rows only 8-byte aligned): one lane per point,
// the rows grid-striding; the interior rows and columns 1..n-1.  false: n too
// large for the partial buffer.
bool launch_raw_step_error(const double *u, const double *h, const double *h2, long n, double p,
                           double w, double atol, double rtol, Rec *partials, Rec *out,
                           hipStream_t s);

// Host: the public record of a device record over interior rows [r0, r1)
void to_step_err(const Rec &r, long n, long r0, long r1, double w, mgx_step_err *out);
// Host: mgx_step_err_merge; false (nothing changed) when the records' w differ
bool merge(mgx_step_err *into, const mgx_step_err &other);
// Host: atol and rtol finite, >= 0 and not both zero
bool tolerances_ok(double atol, double rtol);

// Device time of the calling thread's last error pass and its compulsory bytes
// (tuning keys "errest_us" / "errest_bytes"), the shape of mgxdiag::PassTimer
struct PassTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    void begin(hipStream_t s);
    void end(hipStream_t s);
    void commit(double bytes);   // after the stream has been synchronised
    ~PassTimer();
};
void timer_reset();
void last_pass(double *us, double *bytes);

}  // namespace mgxerr

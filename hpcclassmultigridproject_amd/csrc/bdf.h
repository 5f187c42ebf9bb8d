// bdf.h -- the first pass of a variable-step BDF2 step (csrc/bdf.hip).
//
// mgx_step_bdf2 on a context with a history h = u^(n-1) (mgx_set_history) makes
//     (I + g dt L) u^(n+1) = b0 u^n - b1 u^(n-1) + g dt s f,
// with, all C doubles and every operation rounded (mgx_bdf2_coefficients),
//     w = dt / dt_prev    p = 1 + w        q = 1 + 2 w
//     g = p / q           b0 = (p p) / q   b1 = (w w) / q
//     kA = (2 g) dt       c = (g dt) s
// The solve side is the reference's operator with k = kA; the right-hand side
// is pointwise:
//     rhs(i,j) = fl( fl(b0 u(i,j)) - fl(b1 h(i,j)) )  (then fl(that + fl(c f(i,j))))
// One row march forms it, stores the row of u it holds in registers over the
// row of h it has just read (h becomes u^n, the whole array, ring included --
// u itself is never written) and takes mg_outer's initial norm |rhs - A(kA) u|.
// It is tstep.hip's frame -- grid, per-lane accumulation order, block_sum and
// partial layout of k_res_march<0> -- so the norm is bitwise
// launch_residual_norm's (k = kA) on the stored rhs.
#pragma once
#include <hip/hip_runtime.h>

#include "source.h"

namespace mgxbdf {

struct Coefs {
    double g, b0, b1, kA;
};
// host: the doubles above for a step dt after a step dt_prev
Coefs coefficients(double dt, double dt_prev);

// a: the arguments of the source pass (source.h SrcArgs) -- a.c is the Coef of
// the solve side (kA), a.cf = c; a.f == nullptr and a.terms == 0: no source;
// a.partials / a.norm_out are required; interior rows of [a.ra, a.rb) and
// a.take_sqrt as there.  h: the history, the layout of a.u (h + r*pitch =
// global row r); every row of [a.ra, a.rb) of it is overwritten with u's.
// hin: where u^(n-1) is read -- h itself (a history of depth 1), or the other
// array of a history of depth 2, the same layout.
void launch_rhs_norm_bdf(const mgxsrc::SrcArgs &a, const double *hin, double *h, double b0,
                         double b1, hipStream_t s);

// reference layout (pitch n+1, one point per lane), the gs.h-style raw op: the
// interior of rhs alone is written; f may be null
void launch_raw_rhs_bdf(double *rhs, const double *u, const double *h, long n, double b0,
                        double b1, const double *f, double c, hipStream_t s);

}  // namespace mgxbdf

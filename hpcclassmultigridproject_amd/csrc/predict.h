// predict.h -- the first pass of a BDF2 step with a predicted start
// (mgx_set_predictor; csrc/predict.hip).
//
// The guess g is the dense-output interpolant through u = u^n, h = u^(n-1) (and
// h2 = u^(n-2) at order 2) evaluated one step ahead (dense.h weights, tau =
// +dt): on the interior, every operation rounded and none contracted,
//     e = 1:  g = fl( fl(w0 u) + fl(w1 h) )
//     e = 2:  g = fl( fl( fl(w0 u) + fl(w1 h) ) + fl(w2 h2) )
// and on the ring g = u, the same bits.  One row march in the frame of bdf.hip's
// k_rhs_norm_bdf forms the BDF2 right-hand side (the same bits), g, and the two
// norms |rhs - A u| and |rhs - A g| with the level's coef (k = kA), both in
// launch_residual_norm's grid, per-lane order, block_sum and partial layout --
// the first is bitwise the norm of launch_rhs_norm_bdf.
//
// The pass writes rhs, g and the partial sums and reads everything else: it
// stores no snapshot.  It reads h (and h2) at stencil neighbours that other
// workgroups hold, so the history moves on by an exchange of pointers on the
// host (mgx.hip), never by a store into an array the launch reads.
#pragma once
#include <hip/hip_runtime.h>

#include "source.h"

namespace mgxpred {

// a: the arguments of launch_rhs_norm_bdf (a.c the Coef of the solve side, a.cf
// = c; a.partials: two partial arrays of norm_partials_size() doubles each; the
// whole level, a.ra / a.rb are not read).  a.norm_out[0] = |rhs - A u|,
// a.norm_out[1] = |rhs - A g|.  h, h2 (order 2 only), gout: the layout of a.u;
// gout is written whole (rows 0..n, every column pair up to column n) and is
// none of the arrays read.  w: mgx_dense_weights(order, +dt, ...).
void launch_predict_bdf(const mgxsrc::SrcArgs &a, const double *h, const double *h2, int order,
                        const double w[3], double *gout, double b0, double b1, hipStream_t s);

}  // namespace mgxpred

// tstep.h -- the first pass of a theta-scheme step (csrc/tstep.hip).
//
// mgx_set_time_step(ctx, dt, theta) makes a step
//     (I + theta dt L) u^(n+1) = (I - (1 - theta) dt L) u^n + dt f,
// the reference's two operators built from two different k:
//     A = make_coef(kA, ...),  kA = fl(fl(2 theta) dt)         (solve side)
//     B = make_coef(kB, ...),  kB = fl(fl(2 fl(1 - theta)) dt) (right-hand side)
// Every smoothing, restriction and cross-cycle kernel takes A alone; the one
// pass that needs both is the step's first: rhs = B u (+ the source term) and
// mg_outer's initial norm |rhs - A u|.  The kernels that fuse the two for
// Crank-Nicolson (kernels.hip k_res_march MODE 3, source.hip k_rhs_source) form
// both sides from one Coef, so kA != kB runs this pass instead.
//
// It is source.hip's norm instance with a second Coef: the same frame, grid,
// per-lane accumulation order, block_sum and partial layout as k_res_march<0>,
// so the stored rhs is bitwise mgx_rhs's (k = kB) and the norm bitwise
// launch_residual_norm's (k = kA) on it.  Both point expressions keep the
// reference's term order in either fp_mode (gs.cpp:44, :75).
#pragma once
#include <hip/hip_runtime.h>

#include "source.h"

namespace mgxts {

// a: the arguments of the source pass (source.h SrcArgs) -- a.c is the
// right-hand side's Coef (kB); a.f == nullptr and a.terms == 0: no source;
// a.partials / a.norm_out are required (this pass always takes the norm);
// rows [a.ra, a.rb) and a.take_sqrt as there.  cA: the Coef of the solve side.
void launch_rhs_norm2(const mgxsrc::SrcArgs &a, const mgx::Coef &cA, hipStream_t s);

}  // namespace mgxts

// source.h -- compute_rhs with a source term (csrc/source.hip).
//
// u_t + v.grad u = nu lap u + f: the Crank-Nicolson right-hand side of a step
// becomes, at every interior point,
//     rhs(i,j) = fl( Bu(i,j) + fl( cf * f(i,j) ) ),   cf = fl(dt * scale),
// Bu = compute_rhs (gs.cpp:24-53, stencil.h rhs_point) -- two roundings after
// Bu, never contracted.  One row march over the finest level forms it (the
// MODE 2 / MODE 3 roles of kernels.hip's k_res_march plus the f stream): u,
// v1, v2, f in, rhs out, optionally the sum of squares of rhs - A u.  The norm
// instance uses k_res_march<0>'s grid and partial-sum order, so the norm is
// bitwise launch_residual_norm's on the stored rhs.
//
// A separable source (mgx_set_source_separable) is a short sum of outer
// products given by its factors, 1 <= R <= kMaxTerms terms:
//     f(i,j) = fl( ... fl( fl(t_0 + t_1) + t_2 ) ... ),  t_r = fl(a[r][i] * b[r][j])
// (f = t_0 for R = 1), left to right, every product and sum rounded: bitwise
// the array numpy builds with f = a[0][:,None]*b[0][None,:], then f = f +
// a[r][:,None]*b[r][None,:].  The march forms it in registers: no array, no
// stream, and the norm instance is bitwise that of the field pass on that f.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace mgxsrc {

constexpr int kMaxTerms = 4;   // MGX_SOURCE_MAX_TERMS

struct SrcArgs {
    double *rhs = nullptr;
    const double *u = nullptr, *v1 = nullptr, *v2 = nullptr;
    const double *f = nullptr;   // the source, tower layout (ptr + r*pitch = global row r)
    // terms > 0: a separable source instead of f.  fa + r*(n+1): the row factor
    // of term r, indexed by the global row; fb + r*pitch: its column factor,
    // zero padded to the pitch
    int terms = 0;
    const double *fa = nullptr, *fb = nullptr;
    double cf = 0.0;             // fl(dt * scale)
    long n = 0, pitch = 0;
    mgx::Coef c{};
    // exact velocity factors (sepvel.h), all four set: v1[R][j] = fl(sa1[R] *
    // sb1[j]) bitwise, v2 likewise -- the pass reads them instead of the 2-D
    // v1 / v2 (three full streams instead of five)
    const double *sa1 = nullptr, *sb1 = nullptr, *sa2 = nullptr, *sb2 = nullptr;
    // partials set: also the residual norm against the new rhs, as
    // launch_rhs_norm (norm_partials_size() doubles; *norm_out = sqrt of the
    // sum, or the sum when !take_sqrt)
    double *partials = nullptr, *norm_out = nullptr;
    bool take_sqrt = true;
    int ra = 0, rb = -1;   // output rows [ra, rb) (rb < 0: the whole level), as launch_rhs
};
void launch_rhs_source(const SrcArgs &a, hipStream_t s);
// the grid and rows per group of a norm instance over `rows` interior rows:
// launch_residual_norm's (shared with tstep.hip)
void res_grid(long n, long rows, dim3 &g, int &R);

// reference layout (pitch n+1, one point per lane), the gs.h-style raw op
void launch_raw_rhs_source(double *rhs, const double *u, const double *v1, const double *v2,
                           const double *f, double cf, long n, mgx::Coef c, hipStream_t s);
// the same with a separable source: fa, fb hold terms x (n+1) doubles, term-major
void launch_raw_rhs_source_sep(double *rhs, const double *u, const double *v1, const double *v2,
                               int terms, const double *fa, const double *fb, double cf, long n,
                               mgx::Coef c, hipStream_t s);

}  // namespace mgxsrc

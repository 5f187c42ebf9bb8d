// dense.h -- dense output: the interpolant through the resident time levels at
// a time inside the last step (csrc/dense.hip; include/mgx.h "Dense output").
//
// After a step u = u^(n+1), h = u^n and (depth 2) h2 = u^(n-1) lie in HBM.  With
// tau = t* - t^(n+1) <= 0 and the weights of mgx_dense_weights (host, C doubles,
// every operation rounded), at a point
//     levels 1 (order 0):  out = u                                  the same bits
//     levels 2 (order 1):  out = fl( fl(w0*u) + fl(w1*h) )
//     levels 3 (order 2):  out = fl( fl( fl(w0*u) + fl(w1*h) ) + fl(w2*h2) )
// never contracted (-ffp-contract=off).  `levels` is a template parameter of
// every kernel: levels 2 never touches h2 (the array may not exist), levels 1
// touches neither history array.  No atomics, no reduction.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mgx.h"

namespace mgxdense {

// Host: the weights of mgx_dense_weights into w[3].  0 = fine; 1 = order outside
// 0..2, 2 = tau not finite, 3 = dt1 not finite or <= 0 (order >= 1), 4 = dt2 not
// finite or <= 0 (order 2); w is untouched then.
int weights(int order, double tau, double dt1, double dt2, double w[3]);

// Up to three arrays in one tower layout: element (i, j) at a[(i - row0) * pitch
// + j], pitch % 2 == 0 and the arrays 16-byte aligned; `levels` (1..3) of them
// are read, in the order u, h, h2.
struct Src {
    const double *u = nullptr, *h = nullptr, *h2 = nullptr;
    long row0 = 0, pitch = 0, n = 0;
    int levels = 1;
    double w0 = 1, w1 = 0, w2 = 0;
};

// Row march, the frame of errest.hip's k_err_march (256 lanes = 512 columns per
// workgroup, one column pair per lane, 16-byte loads, four rows in flight):
// out[(i - orow0) * (n + 1) + j] for rows [r0, r1), all columns 0..n.  store:
// the tuning key "dense_store" (0 plain, 1 non-temporal, 2 one 16-byte store per
// pair on every row); group_rows: "dense_rows" (0: the frame's row groups).
void launch_march(const Src &s, long r0, long r1, double *out, long orow0, int store,
                  int group_rows, hipStream_t st);
// out[(A - A0) * ld + B] = interpolant(A * stride, B * stride), A0 <= A < A1,
// 0 <= B <= n / stride: the frame of diag.hip's k_gather
void launch_gather(const Src &s, long stride, long A0, long A1, double *out, long ld,
                   hipStream_t st);
// out[k] = interpolant(pi[k], pj[k]) for the points whose row lies in [ra, rb)
// (the rows the arrays hold).  An index outside 0..n gives NaN and reads
// nothing; a valid point outside [ra, rb) gives NaN where fill_unheld, and is
// left alone otherwise (another launch of a partitioned context writes it).
void launch_points(const Src &s, long ra, long rb, bool fill_unheld, long npts, const long *pi,
                   const long *pj, double *out, hipStream_t st);
// Reference layout (pitch n+1, rows only 8-byte aligned): one lane per point
// over all (n+1)^2, grid-striding
void launch_raw(double *out, const double *u, const double *h, const double *h2, long n, double w0,
                double w1, double w2, int levels, hipStream_t st);

// Device time of the calling thread's last dense call and its compulsory bytes
// (tuning keys "dense_us" / "dense_bytes"), the shape of mgxerr::PassTimer
struct PassTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    void begin(hipStream_t s);
    void end(hipStream_t s);
    void commit(double bytes);   // after the stream has been synchronised
    ~PassTimer();
};
void timer_reset();
void last_pass(double *us, double *bytes);

}  // namespace mgxdense

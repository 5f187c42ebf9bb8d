// vfactor.h -- the device backend of sepvel.h's exact rank-1 factorisation.
//
// mgxsep::factor_rank1_on (sepvel.h) decides on the host; here its three data
// accesses run on a field that lives in device memory: a strided gather of one
// column, copies of the <= 32 pivot rows, and k_vf_check, which streams every
// entry once, compares bits(fl(a[i]*b[j])) with bits(v[i][j]) and sets one
// flag per failing column (and the range flag of the same pass).  The host
// reads back the flags: one synchronisation per round.  Same a, b, jsel bits
// as the host backend for the same field.
#pragma once
#include <hip/hip_runtime.h>

namespace mgxvf {

// v: rows x w, row stride ld doubles, DEVICE memory (any ld >= w; 16-byte
// loads where v and the rows are 16-byte aligned, 8-byte loads otherwise).
// a[rows], b[w]: HOST arrays.  -> 1 factored (a, b, *jsel filled), 0 not
// rank-1 (or out of range under smin), -1 a HIP call failed (*err).
// Work is enqueued on `stream`, which is synchronised before returning.
int factor_rank1_device(const double *v, long rows, long w, long ld, double smin, double *a,
                        double *b, hipStream_t stream, long *jsel, hipError_t *err);

// (statistics of the last call on this thread, for measurements: launches of
// the check kernel and their summed device milliseconds, HIP events)
void last_stats(int *rounds, double *ms);

}  // namespace mgxvf

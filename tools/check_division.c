// check_division.c -- the smoother's division (kernels.hip div_diag) is bitwise IEEE division.
//
// q0 = RN(a*y) with y = RN(1/d), r = fma(-q0, d, a) (exact), q = r == 0 ? q0 : fma(r, y, q0).
// Markstein's theorem says q = RN(a/d) when y = RN(1/d) and q0 is within one ulp; this
// program checks it on random numerators for every diagonal 1-4*rr*nu the solver uses
// (N = 8..65536, all levels, nu in {-4e-4, -0.01}) and on random divisors.
// usage: check_division [samples_per_divisor] [random_divisor_samples]
//
// That holds on a domain.  The proof needs the remainder r = a - q0*d exact.  q0*d has its
// last bit at 2^(e(q0)+e(d)-104) and r is a multiple of it, so r is representable -- in the
// subnormal range at worst -- iff e(q0)+e(d) >= -970; with e(a) = e(q0)+e(d) or one more,
// that is guaranteed for |a| >= 2^-969 and lost, for some a, from the binade [2^-970, 2^-969)
// down: there r is rounded and q may be the neighbour of RN(a/d), one ulp off.  a = +-Inf
// gives r = Inf - Inf = NaN where a/d = +-Inf.  +-0 and NaN agree.  The range mode measures
// this for both forms of csrc/stencil.h div_diag -- POSD (d > 0: rn = fma(q0, d, -a),
// q = fma(-rn, y, q0)) and the general one (sign bit of q set to sign(a) xor sign(d)), the
// latter with d and with -d:
//        check_division range ELO EHI [samples_per_divisor]
// draws |a| from the binades 2^ELO .. 2^EHI (unbiased exponents, -1023 = the subnormals),
// either sign, and prints per form the mismatches against a / d and their largest distance
// in ulp;
//        check_division special
// does the same for a = +-0, NaN and +-Inf.  Both always exit 0: tests/test_division.py
// asserts on the figures.
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
static uint64_t s = 88172645463325252ull;
static inline uint64_t xr(void){ s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static double rnd_double(void){ uint64_t b = xr(); // random finite normal double in moderate range
  uint64_t e = 1023 - 200 + (xr() % 400); b = (b & 0x800FFFFFFFFFFFFFull) | (e << 52); double d; memcpy(&d,&b,8); return d; }
static double mk(int e){ uint64_t b = xr(); b = (b & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(e + 1023) << 52); double d; memcpy(&d,&b,8); return d; }
static double div_posd(double a, double d, double y){ double q0 = a * y; double rn = fma(q0, d, -a); return fma(-rn, y, q0); }
static double div_general(double a, double d, double y){
  double q0 = a * y; double r = fma(-q0, d, a); double q = fma(r, y, q0);
  uint64_t qb, ab, db; memcpy(&qb,&q,8); memcpy(&ab,&a,8); memcpy(&db,&d,8);
  qb = (qb & 0x7fffffffffffffffull) | ((ab ^ db) & 0x8000000000000000ull); memcpy(&q,&qb,8); return q; }
static int64_t ordered(double x){ int64_t i; memcpy(&i,&x,8); return i < 0 ? INT64_MIN - i : i; }
// -> 0 equal bits (or both NaN), else the distance in ulp (a NaN against a number: 1 << 62)
static int64_t ulps(double got, double exp){
  if (got != got || exp != exp) return (got != got && exp != exp) ? 0 : ((int64_t)1 << 62);
  if (!memcmp(&got,&exp,8)) return 0;
  int64_t a = ordered(got), b = ordered(exp), u = a > b ? a - b : b - a; return u ? u : 1; /* (+0 against -0: 1) */ }
static int divisors(double *ds){
  int nd = 0; double nus[2] = {-4e-4, -0.01};   // (the list of main below)
  for (int N = 8; N <= 65536; N *= 2) for (int q = 0; q < 2; q++) {
    double k = (1.0/N)/10; double h = 1.0/N;
    for (int l = 0; (N >> l) >= 2 && nd < 60; l++, h *= 2) { double rr = 0.5*k/(h*h); ds[nd++] = 1.0 - 4.0*rr*nus[q]; if (nd >= 60) break; }
  }
  return nd; }
struct tally { long bad; int64_t max; };
static void count(struct tally *t, double got, double exp){ int64_t u = ulps(got, exp); if (u) { t->bad++; if (u > t->max) t->max = u; } }
static int range_mode(int elo, int ehi, long per){
  double ds[64]; int nd = divisors(ds); long tot = 0; struct tally p = {0,0}, g = {0,0}, n = {0,0};
  for (int i = 0; i < nd; i++) { double d = ds[i], y = 1.0 / d, yn = 1.0 / -d;
    for (long t = 0; t < per; t++) { double a = mk(elo + (int)(xr() % (uint64_t)(ehi - elo + 1))); tot++;
      count(&p, div_posd(a, d, y), a / d); count(&g, div_general(a, d, y), a / d); count(&n, div_general(a, -d, yn), a / -d); } }
  printf("range 2^%d..2^%d: divisors %d, tests %ld, posd mismatches %ld max_ulp %lld, general mismatches %ld max_ulp %lld, "
         "general_negd mismatches %ld max_ulp %lld\n", elo, ehi, nd, tot, p.bad, (long long)p.max, g.bad, (long long)g.max,
         n.bad, (long long)n.max);
  return 0; }
static int special_mode(void){
  double ds[64]; int nd = divisors(ds); long zero_bad = 0, nan_bad = 0, inf_not_nan = 0;
  double zs[2] = {0.0, -0.0}, infs[2] = {INFINITY, -INFINITY};
  for (int i = 0; i < nd; i++) { double d = ds[i], y = 1.0 / d, yn = 1.0 / -d;
    for (int k = 0; k < 2; k++) {
      double a = zs[k];
      zero_bad += (ulps(div_posd(a, d, y), a / d) != 0) + (ulps(div_general(a, d, y), a / d) != 0) + (ulps(div_general(a, -d, yn), a / -d) != 0);
      a = k ? -NAN : NAN;
      nan_bad += (ulps(div_posd(a, d, y), a / d) != 0) + (ulps(div_general(a, d, y), a / d) != 0) + (ulps(div_general(a, -d, yn), a / -d) != 0);
      a = infs[k]; double q;
      q = div_posd(a, d, y); inf_not_nan += q == q; q = div_general(a, d, y); inf_not_nan += q == q; q = div_general(a, -d, yn); inf_not_nan += q == q;
    } }
  printf("special: divisors %d, zero mismatches %ld, nan mismatches %ld, inf results that are not NaN %ld\n", nd, zero_bad, nan_bad, inf_not_nan);
  return 0; }
int main(int argc, char **argv){
  if (argc > 3 && !strcmp(argv[1], "range")) {
    int elo = atoi(argv[2]), ehi = atoi(argv[3]);
    if (elo < -1023 || ehi > 1023 || elo > ehi) { fprintf(stderr, "range: -1023 <= ELO <= EHI <= 1023\n"); return 2; }
    return range_mode(elo, ehi, argc > 4 ? atol(argv[4]) : 20000);
  }
  if (argc > 1 && !strcmp(argv[1], "special")) return special_mode();
  long per = argc > 1 ? atol(argv[1]) : 20000000, rnd = argc > 2 ? atol(argv[2]) : 200000000;
  long bad = 0, tot = 0;
  double ds[64]; int nd = 0;
  // the actual divisors: dgs = 1 - 4*rr*nu for N up to 65536, all levels, nu in {-4e-4,-0.01}
  double nus[2] = {-4e-4, -0.01};
  for (int N = 8; N <= 65536; N *= 2) for (int q = 0; q < 2; q++) {
    double k = (1.0/N)/10; double h = 1.0/N;
    for (int l = 0; (N >> l) >= 2 && nd < 60; l++, h *= 2) { double rr = 0.5*k/(h*h); ds[nd++] = 1.0 - 4.0*rr*nus[q]; if (nd >= 60) break; }
  }
  for (int i = 0; i < nd; i++) {
    double d = ds[i], y = 1.0 / d;
    for (long t = 0; t < per; t++) {
      double a = rnd_double();
      double q0 = a * y; double r = fma(-q0, d, a); double qq = (r == 0.0) ? q0 : fma(r, y, q0);
      double ex = a / d; tot++;
      if (memcmp(&qq, &ex, 8)) { if (bad < 10) printf("MISMATCH d=%.17g a=%.17g got=%.17g exp=%.17g\n", d, a, qq, ex); bad++; }
    }
  }
  // random divisors too
  for (long t = 0; t < rnd; t++) {
    double d = rnd_double(); if (d < 0) d = -d; double y = 1.0/d; double a = rnd_double();
    double q0 = a * y; double r = fma(-q0, d, a); double qq = (r == 0.0) ? q0 : fma(r, y, q0);
    double ex = a / d; tot++;
    if (memcmp(&qq, &ex, 8)) { if (bad < 20) printf("MISMATCH2 d=%.17g a=%.17g got=%.17g exp=%.17g\n", d, a, qq, ex); bad++; }
  }
  printf("divisors %d, tests %ld, mismatches %ld\n", nd, tot, bad);
  return bad != 0;
}

"""The meaning of the step error record (mgx_step_error, include/mgx.h) in
numpy, and the bound its sums are compared by.

All np.float64, every operation rounded, in the order the header states: with
w = dt_prev / dt_prev2 and p = 1 + w, at every interior point

    up = fl( fl(p h) - fl(w h2) )
    d  = fl( u - up )
    c  = fl( u - h )
    sc = fl( atol + fl( rtol max(|u|, |h|) ) )
    e  = d / sc

A point whose e is not finite counts in `nonfinite` alone.  The exact fields
(count, nonfinite, w, the three maxima as bits, the position of the largest
|e|, first occurrence in row-major order) are compared exactly.  The sums of
fl(x x) are compared by Higham's bound for recursive summation in any order,
|got - S| <= (m - 1) u S / (1 - (m - 1) u) <= 2 m 2^-53 S for m non-negative
terms (m 2^-53 < 1/2), with S summed accurately (math.fsum): derived, not
measured -- the bound of tests/test_gpu_stats.py.
"""
import math

import numpy as np

EXACT = ("count", "nonfinite", "w", "err_max", "err_max_i", "err_max_j", "d_max", "c_max")
SUMS = ("err_sum_sq", "d_sum_sq", "c_sum_sq")


def weight(dt_prev, dt_prev2):
    return np.float64(dt_prev) / np.float64(dt_prev2)


def reference(u, h, h2, N, w, atol, rtol, r0=0, r1=None):
    """The record over the interior points of rows [r0, r1) of three flat
    (N+1)^2 arrays -> dict: the exact fields, the accurately summed sums, and
    `m`, the number of finite points."""
    n1 = N + 1
    r1 = n1 if r1 is None else r1
    ra, rb = max(r0, 1), max(max(r0, 1), min(r1, N))
    U, H, H2 = (np.asarray(x, dtype=np.float64).reshape(n1, n1)[ra:rb, 1:N] for x in (u, h, h2))
    w = np.float64(w)
    p = np.float64(1.0) + w
    atol, rtol = np.float64(atol), np.float64(rtol)
    with np.errstate(all="ignore"):
        up = p * H - w * H2
        d = U - up
        c = U - H
        sc = atol + rtol * np.maximum(np.abs(U), np.abs(H))
        e = d / sc
        fin = np.isfinite(e)
        ae = np.where(fin, np.abs(e), -np.inf)
        e2, d2, c2 = e * e, d * d, c * c
    m = int(fin.sum())
    out = {"count": int(U.size), "nonfinite": int(U.size - m), "w": float(w), "m": m}
    if m:
        k = int(np.argmax(ae))          # the first occurrence in row-major order
        i, j = divmod(k, U.shape[1])
        out.update(err_max=float(ae.flat[k]), err_max_i=ra + i, err_max_j=1 + j,
                   d_max=float(np.abs(d[fin]).max()), c_max=float(np.abs(c[fin]).max()))
    else:
        out.update(err_max=-math.inf, err_max_i=-1, err_max_j=-1, d_max=-math.inf,
                   c_max=-math.inf)
    out["err_sum_sq"] = accurate_sum(e2[fin])
    out["d_sum_sq"] = accurate_sum(d2[fin])
    out["c_sum_sq"] = accurate_sum(c2[fin])
    return out


def accurate_sum(x):
    """S of the bound: math.fsum, or from 2^17 terms on numpy's pairwise sum in
    an extended np.longdouble where there is one (64-bit significand: its own
    error, about log2(m) 2^-64 S plus one rounding to double, is far inside the
    bound's slack between m - 1 and 2 m)."""
    if x.size >= 1 << 17 and np.finfo(np.longdouble).nmant >= 63:
        return float(np.sum(x, dtype=np.longdouble))
    return math.fsum(x.tolist())


def bits(x):
    return np.float64(x).view(np.uint64)


def check(got, want, what=""):
    """got: an object with the record's fields (StepError); want: reference()."""
    for f in EXACT:
        g, x = getattr(got, f), want[f]
        same = bits(g) == bits(x) if isinstance(x, float) else g == x
        assert same, (what, f, g, x)
    m = want["m"]
    assert m * 2.0 ** -53 < .5
    for f in SUMS:
        g, S = getattr(got, f), want[f]
        bound = 2.0 * m * 2.0 ** -53 * S
        print(f"{what}: {f} got {g!r} exact {S!r} |diff| {abs(g - S):.3e} bound {bound:.3e}")
        assert abs(g - S) <= bound, (what, f, g, S, bound)
    want_rms = math.sqrt(got.err_sum_sq / m) if m else math.nan
    assert got.rms == want_rms or (math.isnan(got.rms) and math.isnan(want_rms)), (what, got.rms)

"""The meaning of dense output (mgx_dense_weights, mgx_dense_output,
include/mgx.h "Dense output") on the CPU.

weights(): Python floats, which are IEEE doubles -- the rounded operations of
the header in the header's order.  reference(): numpy float64, each operation
rounded once, none fused:

    order 0:  out = u                                        (the same bits)
    order 1:  out = fl( fl(w0 u) + fl(w1 h) )
    order 2:  out = fl( fl( fl(w0 u) + fl(w1 h) ) + fl(w2 h2) )

Everything the device computes is compared with this bit for bit.
"""
import numpy as np


def weights(order, tau, dt1, dt2=0.0):
    tau, dt1, dt2 = float(tau), float(dt1), float(dt2)
    if order == 0:
        return 1.0, 0.0, 0.0
    if order == 1:
        w1 = (0.0 - tau) / dt1
        w0 = 1.0 - w1
        return w0, w1, 0.0
    assert order == 2
    s = dt1 + dt2
    a = tau + dt1
    b = tau + s
    w0 = (a * b) / (dt1 * s)
    w1 = ((0.0 - tau) * b) / (dt1 * dt2)
    w2 = (tau * a) / (s * dt2)
    return w0, w1, w2


def combine(u, h, h2, levels, w0, w1, w2):
    """The point formula on arrays for given weights (the raw op's meaning) ->
    a flat array; the inputs may have any shape of one size."""
    u = np.asarray(u, dtype=np.float64).ravel()
    if levels == 1:
        return u.copy()
    with np.errstate(all="ignore"):
        out = np.float64(w0) * u + np.float64(w1) * np.asarray(h, dtype=np.float64).ravel()
        if levels == 3:
            out = out + np.float64(w2) * np.asarray(h2, dtype=np.float64).ravel()
    return out


def reference(u, h, h2, order, tau, dt1, dt2=0.0):
    return combine(u, h, h2, order + 1, *weights(order, tau, dt1, dt2))


def bits_equal(a, b, nan_bits=False):
    """The same bits everywhere.  Where both entries are NaN the bits are
    compared only with nan_bits (a copy): IEEE 754 leaves the sign and payload
    of a NaN that an operation produces (Inf - Inf, 0 * Inf) to the
    implementation, and the host's and the device's defaults differ in the sign."""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    if a.shape != b.shape:
        return False
    same = a.view(np.uint64) == b.view(np.uint64)
    if not nan_bits:
        same |= np.isnan(a) & np.isnan(b)
    return bool(same.all())

"""The dense output entry points (mgx_dense_weights, mgx_dense_output[_device],
mgx_dense_output_rows, mgx_dense_points[_device], mgx_array_dense) without a
GPU: declared, exported, bound; argument and state errors come back as
MGX_E_ARG with a message that begins with the function's name, before any
device call; the host-only weights against the checker bit for bit; the
accuracy of the scheme through the checker; outputs_between; the Makefile and
the provenance comment list the new sources."""
import ctypes as C
import math
import os
import random
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hpcclassmultigridproject_amd as pkg
from hpcclassmultigridproject_amd import Multigrid, _lib

import dense as D

NEW = ("mgx_dense_weights", "mgx_dense_output", "mgx_dense_output_device",
       "mgx_dense_output_rows", "mgx_dense_points", "mgx_dense_points_device", "mgx_array_dense")
INF, NAN = math.inf, math.nan


def err_arg(name, rc):
    assert rc == _lib.MGX_E_ARG, name
    msg = _lib.lib().mgx_last_error().decode()
    assert re.match(r"%s\b(?!_)" % name, msg), (name, msg)
    return msg


def test_new_symbols_declared_bound_and_exported():
    hdr = open(_lib.HEADER_PATH).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (mgx_\w+)", out))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib._SIGS, name
        assert name in exported, name
    for m in ("dense", "dense_rows", "dense_points"):
        assert callable(getattr(Multigrid, m)), m
    for f in ("dense_weights", "outputs_between"):
        assert callable(getattr(pkg, f)) and f in pkg.__all__, f
    assert callable(_lib.array_dense)
    # provenance and accounting
    block = re.search(r"/\* Build provenance.*?\*/", hdr, re.S).group(0)
    assert "dense.h," in block and "dense.hip" in block
    assert block.index("errest.hip") < block.index("dense.h,") < block.index("dense.hip")
    assert '"dense_us"' in hdr and '"dense_bytes"' in hdr
    assert re.search(r"#define\s+MGX_K_COUNT\s+9\b", hdr)
    for key in ("dense_us", "dense_bytes"):
        assert _lib.get_tuning(key) >= 0
        with pytest.raises(_lib.MGXError):
            _lib.set_tuning(key, 1)


def test_makefile_lists_the_new_sources():
    mk = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc",
                           "Makefile")).read()
    asha = re.search(r"^ASHA\s*:=(.*?)\n\S", mk, re.M | re.S).group(1).split()
    assert asha.index("errest.hip") < asha.index("dense.h") < asha.index("dense.hip")
    srcs = re.search(r"^SRCS\s*:=(.*?)\n\S", mk, re.M | re.S).group(1)
    merged = re.search(r"^MERGED\s*:=\s*(.*)$", mk, re.M).group(1)
    hdrs = re.search(r"^HDRS\s*:=\s*(.*)$", mk, re.M).group(1)
    assert "dense.hip" in srcs and "dense.hip" in merged
    assert "dense.h" in hdrs.replace("dense.hip", "")
    assert "-ffp-contract=off" in mk


def _calls(lib, ctx, order, tau, stride, out, idx, npts=1):
    """Every context entry point with the given arguments."""
    fr, rows = C.c_long(), C.c_long()
    return {
        "mgx_dense_output": lambda: lib.mgx_dense_output(ctx, order, tau, stride, out),
        "mgx_dense_output_device": lambda: lib.mgx_dense_output_device(ctx, order, tau, stride,
                                                                       out),
        "mgx_dense_output_rows": lambda: lib.mgx_dense_output_rows(
            ctx, 0, order, tau, stride, out, C.byref(fr), C.byref(rows)),
        "mgx_dense_points": lambda: lib.mgx_dense_points(ctx, order, tau, npts, idx, idx, out),
        "mgx_dense_points_device": lambda: lib.mgx_dense_points_device(ctx, order, tau, npts, idx,
                                                                       idx, out),
    }


def test_bad_arguments_return_status_without_a_device():
    """On a handle that is not a context (zero bytes: N = 0, no history) -- the
    checks come before any device call."""
    lib = _lib.lib()
    fake = C.create_string_buffer(1 << 16)
    buf = (C.c_double * 4)()
    idx = (C.c_long * 4)()
    out, ix = C.addressof(buf), C.addressof(idx)
    # a NULL context
    for name, call in _calls(lib, None, 0, 0.0, 1, out, ix).items():
        err_arg(name, call())
    # a NULL out (the rows form: a NULL first_row / rows -- its out may be NULL)
    for name, call in _calls(lib, fake, 0, 0.0, 1, None, ix).items():
        if name != "mgx_dense_output_rows":
            err_arg(name, call())
    err_arg("mgx_dense_output_rows",
            lib.mgx_dense_output_rows(fake, 0, 0, 0.0, 1, out, None, None))
    # the order
    for order in (-1, 3):
        for name, call in _calls(lib, fake, order, 0.0, 1, out, ix).items():
            assert "order" in err_arg(name, call())
    # tau
    for tau in (NAN, INF, -INF):
        for name, call in _calls(lib, fake, 0, tau, 1, out, ix).items():
            assert "tau" in err_arg(name, call())
    # the stride (the calls that take one)
    for stride in (0, -2):
        for name, call in _calls(lib, fake, 0, 0.0, stride, out, ix).items():
            if "points" not in name:
                assert "stride" in err_arg(name, call())
    # state: no history on this handle
    for order in (1, 2):
        for name, call in _calls(lib, fake, order, 0.0, 1, out, ix).items():
            assert "history" in err_arg(name, call())
    # npts < 0; npts = 0 is a no-op whatever the pointers are
    for name in ("mgx_dense_points", "mgx_dense_points_device"):
        err_arg(name, getattr(lib, name)(fake, 0, 0.0, -1, ix, ix, out))
        assert getattr(lib, name)(fake, 0, 0.0, 0, None, None, None) == _lib.MGX_OK
    # the raw op
    for call in (lambda: lib.mgx_array_dense(None, 8, 8, 8, 8, 1.0, 0.0, 0.0, 3),
                 lambda: lib.mgx_array_dense(8, None, 8, 8, 8, 1.0, 0.0, 0.0, 1),
                 lambda: lib.mgx_array_dense(8, 8, None, 8, 8, 1.0, 0.0, 0.0, 2),
                 lambda: lib.mgx_array_dense(8, 8, 8, None, 8, 1.0, 0.0, 0.0, 3),
                 lambda: lib.mgx_array_dense(8, 8, 8, 8, 0, 1.0, 0.0, 0.0, 3),
                 lambda: lib.mgx_array_dense(8, 8, 8, 8, 8, 1.0, 0.0, 0.0, 0),
                 lambda: lib.mgx_array_dense(8, 8, 8, 8, 8, 1.0, 0.0, 0.0, 4)):
        err_arg("mgx_array_dense", call())


def test_points_outside_the_grid_are_named():
    """(N = 0 on the zeroed handle: only (0, 0) is a point)"""
    lib = _lib.lib()
    fake = C.create_string_buffer(1 << 16)
    buf = (C.c_double * 3)()
    pi, pj = (C.c_long * 3)(0, 0, 1), (C.c_long * 3)(0, 0, 0)
    msg = err_arg("mgx_dense_points", lib.mgx_dense_points(
        fake, 0, 0.0, 3, C.addressof(pi), C.addressof(pj), C.addressof(buf)))
    assert "k = 2" in msg, msg
    pi, pj = (C.c_long * 3)(0, 0, 0), (C.c_long * 3)(0, -1, 0)
    msg = err_arg("mgx_dense_points", lib.mgx_dense_points(
        fake, 0, 0.0, 3, C.addressof(pi), C.addressof(pj), C.addressof(buf)))
    assert "k = 1" in msg, msg


def c_weights(order, tau, dt1, dt2):
    return pkg.dense_weights(order, tau, dt1, dt2)


def test_weights_are_the_checkers_bits():
    rng = random.Random(20261021)
    for _ in range(2000):
        dt1 = rng.uniform(1e-4, 1.0)
        dt2 = dt1 / rng.uniform(0.2, 5.0)
        # inside the last step, inside the step before it, and a little outside
        tau = -rng.uniform(0.0, 1.2) * (dt1 + dt2)
        for order in (0, 1, 2):
            got, want = c_weights(order, tau, dt1, dt2), D.weights(order, tau, dt1, dt2)
            assert D.bits_equal(got, want, nan_bits=True), (order, tau, dt1, dt2, got, want)
    # NULL output pointers
    lib = _lib.lib()
    assert lib.mgx_dense_weights(2, -.1, .5, .25, None, None, None) == _lib.MGX_OK
    w1 = C.c_double()
    assert lib.mgx_dense_weights(2, -.1, .5, .25, None, C.byref(w1), None) == _lib.MGX_OK
    assert w1.value == D.weights(2, -.1, .5, .25)[1]


def test_weights_hand_cases():
    for dt1, dt2 in ((.5, .25), (.1, .3), (1e-3, 7e-4)):
        for order in (0, 1, 2):
            assert c_weights(order, 0.0, dt1, dt2) == (1.0, 0.0, 0.0), (order, dt1, dt2)
        assert c_weights(1, -dt1, dt1, dt2) == (0.0, 1.0, 0.0)
    # the nodes of the quadratic, on dyadic steps (every operation exact)
    assert c_weights(2, -.5, .5, .25) == (0.0, 1.0, 0.0)
    assert c_weights(2, -.75, .5, .25) == (0.0, 0.0, 1.0)
    # a bad dt1 / dt2 is refused at exactly the orders that use it
    lib = _lib.lib()
    w = [C.c_double() for _ in range(3)]
    refs = [C.byref(x) for x in w]
    for bad in (0.0, -1.0, NAN, INF, -INF):
        assert lib.mgx_dense_weights(0, -.1, bad, bad, *refs) == _lib.MGX_OK
        assert "dt1" in err_arg("mgx_dense_weights", lib.mgx_dense_weights(1, -.1, bad, .5, *refs))
        assert "dt1" in err_arg("mgx_dense_weights", lib.mgx_dense_weights(2, -.1, bad, .5, *refs))
        assert lib.mgx_dense_weights(1, -.1, .5, bad, *refs) == _lib.MGX_OK
        assert "dt2" in err_arg("mgx_dense_weights", lib.mgx_dense_weights(2, -.1, .5, bad, *refs))
    for order in (-1, 3):
        assert "order" in err_arg("mgx_dense_weights",
                                  lib.mgx_dense_weights(order, -.1, .5, .5, *refs))
    for tau in (NAN, INF, -INF):
        for order in (0, 1, 2):
            assert "tau" in err_arg("mgx_dense_weights",
                                    lib.mgx_dense_weights(order, tau, .5, .5, *refs))
    # extrapolation is not refused
    assert lib.mgx_dense_weights(2, .25, .5, .5, *refs) == _lib.MGX_OK
    assert lib.mgx_dense_weights(1, -3.0, .5, .5, *refs) == _lib.MGX_OK


def test_the_scheme_reproduces_polynomials_of_its_degree():
    """Three levels sampled from A + B t + C t^2, everything a dyadic rational
    small enough that the samples are exact doubles.  Order 2 reproduces the
    polynomial at any tau within 16 * 2^-53 * (|w0 u| + |w1 h| + |w2 h2|): each
    weight carries at most five roundings (two sums, two products, a
    division), then come three products and two sums -- at most eight roundings
    on any term, (1 + 2^-53)^8 - 1 < 16 * 2^-53 with room; order 1 the same
    with C = 0.

    The derivation needs every weight's error to be RELATIVE to the weight.  At
    order 2 it is (dt1, dt2 and their sum are exact here; tau + dt1 and tau + s
    are one rounding each of exact operands).  At order 1, w0 = fl(1 - w1)
    inherits the absolute error 2^-53 w1 of w1: relative to w0 that is at most
    2^-53 while w1 <= 1/2 (then w0 >= w1), so tau in [-dt1/2, 0] is checked by
    the bound above.  Nearer to the old level (w1 > 1/2, w0 -> 0) the inherited
    term 2^-53 |w1 u| is no longer covered by |w0 u| + |w1 h| where |h| << |u|
    -- a property of the formula, not of an implementation -- so tau in [-dt1,
    -dt1/2) is checked with that one term added, 2 * 2^-53 |w1 u|."""
    rng = np.random.default_rng(15)
    pyr = random.Random(15)

    def dy(lo, hi, q):   # a dyadic rational with q fractional bits
        return Fraction(pyr.randint(int(lo * 2 ** q), int(hi * 2 ** q)), 2 ** q)

    for case in range(200):
        dt1, dt2 = dy(1 / 16, 1, 6), dy(1 / 16, 1, 6)
        if not Fraction(1, 5) <= dt1 / dt2 <= 5:
            continue
        t1 = dy(0, 4, 6)
        m = 64
        A = [Fraction(int(x), 256) for x in rng.integers(-1024, 1025, m)]
        B = [Fraction(int(x), 256) for x in rng.integers(-1024, 1025, m)]
        for order in (1, 2):
            Cq = [Fraction(int(x), 256) if order == 2 else Fraction(0)
                  for x in rng.integers(-1024, 1025, m)]

            def poly(t):
                vals = [a + b * t + c * t * t for a, b, c in zip(A, B, Cq)]
                out = np.array([float(v) for v in vals])
                assert all(Fraction(float(v)) == v for v in vals)   # the samples are exact
                return vals, out

            _, u = poly(t1)
            _, h = poly(t1 - dt1)
            _, h2 = poly(t1 - dt1 - dt2)
            for draw in range(4):
                if order == 2:
                    tau = -pyr.uniform(0.0, 1.0) * float(dt1 + dt2)
                else:   # two draws in the near half of the step, two in the far half
                    tau = -pyr.uniform(0.0, 0.5) * float(dt1) - (draw // 2) * float(dt1) / 2
                    assert (draw < 2) == (-tau / float(dt1) <= 0.5)
                w = D.weights(order, tau, float(dt1), float(dt2))
                got = D.reference(u, h, h2, order, tau, float(dt1), float(dt2))
                exact, _ = ([a + b * (t1 + Fraction(tau)) + c * (t1 + Fraction(tau)) ** 2
                             for a, b, c in zip(A, B, Cq)], None)
                for k in range(m):
                    mag = abs(Fraction(w[0]) * Fraction(u[k])) + abs(Fraction(w[1]) *
                                                                     Fraction(h[k]))
                    if order == 2:
                        mag += abs(Fraction(w[2]) * Fraction(h2[k]))
                    bound = 16 * Fraction(1, 2 ** 53) * mag
                    if order == 1 and draw >= 2:
                        bound += 2 * Fraction(1, 2 ** 53) * abs(Fraction(w[1]) * Fraction(u[k]))
                    err = abs(Fraction(float(got[k])) - exact[k])
                    assert err <= bound, (case, order, k, tau, float(err), float(bound))


def test_outputs_between():
    ob = pkg.outputs_between
    t_eval = [0.0, 0.25, 0.5, 0.5625, 0.75, 1.0]
    # the end points: t_old is excluded, t_new included
    assert ob(0.0, 0.25, t_eval) == [(1, 0.0)]
    assert ob(0.25, 0.5, t_eval) == [(2, 0.0)]
    assert ob(-1.0, 0.0, t_eval) == [(0, 0.0)]
    # an empty interval
    assert ob(0.25, 0.375, t_eval) == []
    assert ob(1.0, 2.0, t_eval) == []
    assert ob(0.5, 0.5, t_eval) == []
    assert ob(0.0, 1.0, []) == []
    # several outputs in one step, tau = t_eval - t_new <= 0
    assert ob(0.375, 0.875, t_eval) == [(2, -0.375), (3, -0.3125), (4, -0.125)]
    # consecutive steps hand every entry out exactly once
    ts = [0.0, 0.3, 0.5, 0.55, 0.8, 1.0, 1.3]
    seen = [k for a, b in zip(ts, ts[1:]) for k, _ in ob(a, b, t_eval)]
    assert seen == [1, 2, 3, 4, 5]
    tup = tuple(t_eval)
    assert ob(0.375, 0.875, tup) == ob(0.375, 0.875, t_eval)
    assert ob(0.375, 0.875, np.array(t_eval)) == ob(0.375, 0.875, t_eval)

"""The step error entry points (mgx_set_history_depth, mgx_history_depth,
mgx_step_error, mgx_step_error_rows, mgx_step_err_merge, mgx_array_step_error)
without a GPU: declared, exported, bound; argument and state errors come back
as MGX_E_ARG with a message that begins with the function's name, before any
device call; the host-only merge and next_dt on hand-made values; the Makefile
and the provenance comment list the new sources."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

import hpcclassmultigridproject_amd as pkg
from hpcclassmultigridproject_amd import Multigrid, _lib

NEW = ("mgx_set_history_depth", "mgx_history_depth", "mgx_step_error", "mgx_step_error_rows",
       "mgx_step_err_merge", "mgx_array_step_error")
INF, NAN = math.inf, math.nan
BAD_TOL = ((-1.0, 1.0), (1.0, -1.0), (NAN, 1.0), (1.0, NAN), (INF, 1.0), (1.0, INF), (0.0, 0.0))


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
    for m in ("set_history_depth", "history_depth", "step_error", "step_error_rows"):
        assert callable(getattr(Multigrid, m)), m
    for f in ("next_dt", "step_err_merge"):
        assert callable(getattr(pkg, f)) and f in pkg.__all__, f
    assert callable(_lib.array_step_error)
    assert Multigrid._FIELDS["history"] == 5 and Multigrid._FIELDS["history2"] == 6
    # the struct of the header, field for field
    body = re.search(r"typedef struct mgx_step_err \{(.*?)\} mgx_step_err;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f for f, _ in _lib.StepErr._fields_]
    assert C.sizeof(_lib.StepErr) == 8 * len(names)
    # provenance and accounting
    block = re.search(r"/\* Build provenance.*?\*/", hdr, re.S).group(0)
    assert "errest.h," in block and "errest.hip" in block
    assert '"errest_us"' in hdr and '"errest_bytes"' in hdr
    assert re.search(r"#define\s+MGX_K_COUNT\s+9\b", hdr)
    for key in ("errest_us", "errest_bytes"):
        assert _lib.get_tuning(key) >= 0
        with pytest.raises(_lib.MGXError):
            _lib.set_tuning(key, 1)


def test_null_handles_and_bad_tolerances_return_status_without_a_device():
    lib = _lib.lib()
    s = _lib.StepErr()
    i, d = C.c_int(), C.c_double()
    fake = C.create_string_buffer(1 << 16)
    calls = {
        "mgx_set_history_depth": [lambda: lib.mgx_set_history_depth(None, 2),
                                  lambda: lib.mgx_set_history_depth(None, 0)],
        "mgx_history_depth": [lambda: lib.mgx_history_depth(None, C.byref(i), C.byref(i),
                                                            C.byref(d)),
                              lambda: lib.mgx_history_depth(None, None, None, None)],
        "mgx_step_error": [lambda: lib.mgx_step_error(None, 1e-3, 1e-3, C.byref(s)),
                           lambda: lib.mgx_step_error(fake, 1e-3, 1e-3, None)],
        "mgx_step_error_rows": [lambda: lib.mgx_step_error_rows(None, 0, 1e-3, 1e-3, C.byref(s)),
                                lambda: lib.mgx_step_error_rows(fake, 0, 1e-3, 1e-3, None)],
        "mgx_step_err_merge": [lambda: lib.mgx_step_err_merge(None, C.byref(s)),
                               lambda: lib.mgx_step_err_merge(C.byref(s), None)],
        "mgx_array_step_error": [
            lambda: lib.mgx_array_step_error(None, None, None, 8, 1.0, 1e-3, 1e-3, C.byref(s)),
            lambda: lib.mgx_array_step_error(8, 8, 8, 8, 1.0, 1e-3, 1e-3, None),
            lambda: lib.mgx_array_step_error(8, 8, 8, 1, 1.0, 1e-3, 1e-3, C.byref(s)),   # n < 2
            lambda: lib.mgx_array_step_error(8, 8, 8, 8, NAN, 1e-3, 1e-3, C.byref(s))],
    }
    assert set(calls) == set(NEW)
    for name, cs in calls.items():
        for call in cs:
            err_arg(name, call())
    for atol, rtol in BAD_TOL:
        msg = err_arg("mgx_step_error", lib.mgx_step_error(fake, atol, rtol, C.byref(s)))
        assert "atol" in msg, msg
        msg = err_arg("mgx_step_error_rows",
                      lib.mgx_step_error_rows(fake, 0, atol, rtol, C.byref(s)))
        assert "atol" in msg, msg
        msg = err_arg("mgx_array_step_error",
                      lib.mgx_array_step_error(8, 8, 8, 8, 1.0, atol, rtol, C.byref(s)))
        assert "atol" in msg, msg


def test_state_errors_come_before_the_context_is_touched():
    """On a handle that is not a context (zero bytes: no history, nothing
    valid) -- the checks come before any device call."""
    lib = _lib.lib()
    fake = C.create_string_buffer(1 << 16)
    s = _lib.StepErr()
    for depth in (3, -1):
        msg = err_arg("mgx_set_history_depth", lib.mgx_set_history_depth(fake, depth))
        assert "depth" in msg
    # depth 0 on a context without a history: nothing to do, nothing touched
    assert lib.mgx_set_history_depth(fake, 0) == _lib.MGX_OK
    depth, v2, dt2 = C.c_int(7), C.c_int(7), C.c_double(7.0)
    assert lib.mgx_history_depth(fake, C.byref(depth), C.byref(v2), C.byref(dt2)) == _lib.MGX_OK
    assert (depth.value, v2.value, dt2.value) == (0, 0, 0.0)
    assert lib.mgx_history_depth(fake, None, None, None) == _lib.MGX_OK
    msg = err_arg("mgx_step_error", lib.mgx_step_error(fake, 1e-3, 0.0, C.byref(s)))
    assert "history" in msg, msg
    msg = err_arg("mgx_step_error_rows", lib.mgx_step_error_rows(fake, 0, 0.0, 1e-3, C.byref(s)))
    assert "history" in msg, msg


def rec(count, nonfinite, w, esq, emx, i, j, dsq, dmx, csq, cmx):
    return _lib.StepErr(count, nonfinite, w, esq, emx, i, j, dsq, dmx, csq, cmx)


def test_merge_on_hand_made_records():
    a = rec(10, 1, .5, 2.0, 3.0, 4, 7, 1.0, .25, 8.0, 6.0)
    # equal err_max: the smaller (i, j) wins, whichever side it comes from
    for other, pos in ((rec(5, 0, .5, 1.0, 3.0, 4, 6, .5, .125, 2.0, 7.0), (4, 6)),
                       (rec(5, 0, .5, 1.0, 3.0, 5, 0, .5, .125, 2.0, 7.0), (4, 7)),
                       (rec(5, 0, .5, 1.0, 3.0, 3, 9, .5, .125, 2.0, 7.0), (3, 9))):
        for x, y in ((a, other), (other, a)):
            m = _lib.step_err_merge(x, y)
            assert (m.err_max, m.err_max_i, m.err_max_j) == (3.0,) + pos, (m, pos)
            assert (m.count, m.nonfinite, m.w) == (15, 1, .5)
            assert (m.err_sum_sq, m.d_sum_sq, m.c_sum_sq) == (3.0, 1.5, 10.0)
            assert (m.d_max, m.c_max) == (.25, 7.0)
    # a larger value wins wherever it lies
    m = _lib.step_err_merge(a, rec(1, 0, .5, 16.0, 4.0, 9, 9, 0.0, 0.0, 0.0, 0.0))
    assert (m.err_max, m.err_max_i, m.err_max_j, m.d_max, m.c_max) == (4.0, 9, 9, .25, 6.0)
    # a record without a finite point leaves the other's maxima alone
    empty = rec(3, 3, .5, 0.0, -INF, -1, -1, 0.0, -INF, 0.0, -INF)
    for x, y in ((a, empty), (empty, a)):
        m = _lib.step_err_merge(x, y)
        assert (m.count, m.nonfinite) == (13, 4)
        assert (m.err_max, m.err_max_i, m.err_max_j, m.d_max, m.c_max) == (3.0, 4, 7, .25, 6.0)
        assert (m.err_sum_sq, m.d_sum_sq, m.c_sum_sq) == (2.0, 1.0, 8.0)
    m = _lib.step_err_merge(empty, empty)
    assert (m.count, m.nonfinite, m.err_max, m.err_max_i, m.d_max) == (6, 6, -INF, -1, -INF)
    assert math.isnan(m.rms)
    # neither argument is changed; rms
    assert a.count == 10 and a.err_max_j == 7
    assert _lib.StepError(a).rms == math.sqrt(2.0 / 9)
    # unequal w: refused, nothing changed
    lib = _lib.lib()
    into, other = _lib.StepErr.from_buffer_copy(a), rec(5, 0, .75, 1.0, 9.0, 0, 0, 1.0, 1.0, 1.0, 1.0)
    before = bytes(into)
    msg = err_arg("mgx_step_err_merge", lib.mgx_step_err_merge(C.byref(into), C.byref(other)))
    assert "w" in msg and bytes(into) == before
    with pytest.raises(_lib.MGXError):
        _lib.step_err_merge(a, other)


def test_next_dt_at_its_clamps():
    nd = pkg.next_dt
    assert nd(.1, 1.0, 2) == .1 * .9
    assert nd(.1, 0.0, 2) == .1 * 2.0                       # err == 0: fmax
    assert nd(.1, 1e-12, 2) == .1 * 2.0                     # clamped above
    assert nd(.1, 1e12, 2) == .1 * .2                       # clamped below
    for bad in (NAN, INF, -INF):
        assert nd(.1, bad, 2) == .1 * .2                    # non-finite: fmin
    assert nd(.1, 4.0, 2) == .1 * (.9 * 4.0 ** -.5)
    assert nd(.1, 8.0, 3, safety=1.0) == .1 * 8.0 ** (-1.0 / 3)
    assert nd(.1, 1e-12, 1, fmax=5.0) == .5 and nd(.1, 1e12, 1, fmin=.5) == .05
    assert nd(2.0, .25, 1, safety=1.0, fmax=10.0) == 8.0


def test_makefile_lists_the_new_sources():
    mk = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc",
                           "Makefile")).read()
    ksrc = re.search(r"^KSRC\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert ksrc == ["stencil.h", "kernels.h", "kernels.hip", "wsmooth.hip", "xsmooth.hip"]
    asha = re.search(r"^ASHA\s*:=(.*?)\n\S", mk, re.M | re.S).group(1).split()
    assert "errest.h" in asha and "errest.hip" in asha
    srcs = re.search(r"^SRCS\s*:=(.*?)\n\S", mk, re.M | re.S).group(1)
    merged = re.search(r"^MERGED\s*:=\s*(.*)$", mk, re.M).group(1)
    hdrs = re.search(r"^HDRS\s*:=\s*(.*)$", mk, re.M).group(1)
    assert "errest.hip" in srcs and "errest.hip" in merged
    assert "errest.h" in hdrs.replace("errest.hip", "")

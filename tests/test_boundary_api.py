"""The boundary entry points (mgx_set_boundary and friends) without a GPU:
declared, exported, bound; argument errors come back as MGX_E_ARG with a
message that begins with the function's name, before any device call; the
Makefile lists the new sources and leaves KSRC alone."""
import ctypes as C
import os
import re
import subprocess

import pytest

from hpcclassmultigridproject_amd import Multigrid, _lib

NEW = ("mgx_set_boundary", "mgx_set_boundary_device", "mgx_get_boundary",
       "mgx_get_boundary_device", "mgx_boundary_info", "mgx_write_boundary")


def test_new_symbols_declared_bound_and_exported():
    hdr = open(_lib.HEADER_PATH).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (mgx_\w+)", out))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib._SIGS, name
        assert name in exported, name
    assert re.search(r"#define\s+MGX_BC_NOW\s+0\b", hdr)
    assert re.search(r"#define\s+MGX_BC_NEXT_STEP\s+1\b", hdr)
    assert (_lib.BC_NOW, _lib.BC_NEXT_STEP) == (0, 1)
    assert '"boundary_us"' in hdr
    for m in ("set_boundary", "get_boundary", "boundary_pending"):
        assert callable(getattr(Multigrid, m)), m
    assert callable(_lib.write_boundary)
    # the provenance comment names the new files
    block = re.search(r"/\* Build provenance.*?\*/", hdr, re.S).group(0)
    assert "boundary.h," in block and "boundary.hip" in block


def test_bad_arguments_return_status_without_a_device():
    lib = _lib.lib()
    p = C.c_int()
    calls = {
        "mgx_set_boundary": [lambda: lib.mgx_set_boundary(None, 8, _lib.BC_NOW),
                             lambda: lib.mgx_set_boundary(None, None, _lib.BC_NEXT_STEP)],
        "mgx_set_boundary_device": [lambda: lib.mgx_set_boundary_device(None, 8, _lib.BC_NOW),
                                    lambda: lib.mgx_set_boundary_device(None, None, 7)],
        "mgx_get_boundary": [lambda: lib.mgx_get_boundary(None, 8)],
        "mgx_get_boundary_device": [lambda: lib.mgx_get_boundary_device(None, 8)],
        "mgx_boundary_info": [lambda: lib.mgx_boundary_info(None, C.byref(p))],
        "mgx_write_boundary": [lambda: lib.mgx_write_boundary(None, 8, 8),
                               lambda: lib.mgx_write_boundary(8, 8, None),
                               lambda: lib.mgx_write_boundary(8, 0, 8)],   # n = 0
    }
    assert set(calls) == set(NEW)
    for name, cs in calls.items():
        for call in cs:
            assert call() == _lib.MGX_E_ARG, name
            msg = lib.mgx_last_error().decode()
            assert re.match(r"%s\b(?!_)" % name, msg), (name, msg)


def test_boundary_us_is_read_only():
    assert _lib.get_tuning("boundary_us") >= 0
    with pytest.raises(_lib.MGXError):
        _lib.set_tuning("boundary_us", 1)


def test_makefile_lists_the_new_sources():
    mk = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc",
                           "Makefile")).read()
    ksrc = re.search(r"^KSRC\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert ksrc == ["stencil.h", "kernels.h", "kernels.hip", "wsmooth.hip", "xsmooth.hip"]
    asha = re.search(r"^ASHA\s*:=(.*?)\n\S", mk, re.M | re.S).group(1).split()
    assert "boundary.h" in asha and "boundary.hip" in asha
    srcs = re.search(r"^SRCS\s*:=(.*?)\n\S", mk, re.M | re.S).group(1)
    merged = re.search(r"^MERGED\s*:=\s*(.*)$", mk, re.M).group(1)
    hdrs = re.search(r"^HDRS\s*:=\s*(.*)$", mk, re.M).group(1)
    assert "boundary.hip" in srcs and "boundary.hip" in merged and "boundary.h" in hdrs.replace(
        "boundary.hip", "")
    assert re.search(r"#define\s+MGX_K_COUNT\s+9\b", open(_lib.HEADER_PATH).read())

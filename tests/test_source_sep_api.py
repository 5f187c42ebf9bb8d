"""The separable and row-block source entry points (mgx_set_source_separable,
mgx_set_source_rows and friends), without a GPU: declared, exported, bound, and
argument errors come back as MGX_E_ARG with the function's own name before any
device call."""
import re
import subprocess

from hpcclassmultigridproject_amd import Multigrid, _lib

NEW = ("mgx_set_source_separable", "mgx_set_source_separable_device", "mgx_set_source_rows",
       "mgx_set_source_rows_device", "mgx_source_kind", "mgx_compute_rhs_source_separable")


def test_new_symbols_declared_bound_and_exported():
    hdr = open(_lib.HEADER_PATH).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (mgx_\w+)", out))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib._SIGS, name
        assert name in exported, name
    for m in ("set_source_separable", "set_source_rows", "source_kind"):
        assert callable(getattr(Multigrid, m)), m
    assert callable(_lib.compute_rhs_source_separable)


def _starts_with(name):
    msg = _lib.lib().mgx_last_error().decode()
    assert re.match(r"%s\b(?!_)" % name, msg), (name, msg)


def test_null_arguments_return_status_without_a_device():
    lib = _lib.lib()
    calls = {
        "mgx_set_source_separable": lambda: lib.mgx_set_source_separable(None, 1, 8, 8),
        "mgx_set_source_separable_device":
            lambda: lib.mgx_set_source_separable_device(None, 1, 8, 8),
        "mgx_set_source_rows": lambda: lib.mgx_set_source_rows(None, None),
        "mgx_set_source_rows_device": lambda: lib.mgx_set_source_rows_device(None, None),
        "mgx_source_kind": lambda: lib.mgx_source_kind(None, None, None),
        "mgx_compute_rhs_source_separable": lambda: lib.mgx_compute_rhs_source_separable(
            None, None, 8, None, None, 0.1, 0.0, 0.1, 1, None, None, 1.0),
    }
    for name, call in calls.items():
        assert call() == _lib.MGX_E_ARG, name
        _starts_with(name)
    # each null pointer of the raw op on its own (dummy non-null others)
    for k in (0, 1, 3, 4, 9, 10):
        args = [8, 8, 8, 8, 8, 0.1, 0.0, 0.1, 1, 8, 8, 1.0]
        args[k] = None
        assert lib.mgx_compute_rhs_source_separable(*args) == _lib.MGX_E_ARG, k
        _starts_with("mgx_compute_rhs_source_separable")


def test_raw_op_refuses_bad_terms_and_n():
    """terms outside 1..4 and n = 1 (no interior point): dummy non-null
    pointers, refused before any device call."""
    lib = _lib.lib()
    for terms, n in ((0, 8), (5, 8), (-1, 8), (1, 1), (2, 0)):
        rc = lib.mgx_compute_rhs_source_separable(8, 8, n, 8, 8, 0.1, 0.0, 0.1, terms, 8, 8, 1.0)
        assert rc == _lib.MGX_E_ARG, (terms, n)
        _starts_with("mgx_compute_rhs_source_separable")


def test_max_terms_constant():
    hdr = open(_lib.HEADER_PATH).read()
    m = re.search(r"^#define\s+MGX_SOURCE_MAX_TERMS\s+(\d+)\s*$", hdr, re.M)
    assert m and int(m.group(1)) == 4
    assert _lib.MGX_SOURCE_MAX_TERMS == 4

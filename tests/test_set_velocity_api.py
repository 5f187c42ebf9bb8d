"""The velocity-replacement and device-factorisation entry points, without a
GPU: declared, exported, bound, and argument errors come back as a status
before any device call."""
import re
import subprocess

import pytest

from hpcclassmultigridproject_amd import Multigrid, _lib

NEW = ("mgx_factor_velocity_device", "mgx_set_velocity", "mgx_set_velocity_device")


def test_new_symbols_declared_bound_and_exported():
    hdr = open(_lib.HEADER_PATH).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (mgx_\w+)", out))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib._SIGS, name
        assert name in exported, name
    assert callable(Multigrid.set_velocity)
    assert callable(_lib.factor_velocity_device)


def test_null_arguments_return_status_without_a_device():
    lib = _lib.lib()
    assert lib.mgx_set_velocity(None, None, None) == _lib.MGX_E_ARG
    assert "mgx_set_velocity" in lib.mgx_last_error().decode()
    assert lib.mgx_set_velocity_device(None, None, None) == _lib.MGX_E_ARG
    assert lib.mgx_factor_velocity_device(None, 1, 1, 2, 0.0, None, None, None) == _lib.MGX_E_ARG


def test_device_factor_key():
    assert '"device_factor"' in open(_lib.HEADER_PATH).read()
    old = _lib.get_tuning("device_factor")
    assert old == 1
    try:
        for v in (0, 2, 1):
            _lib.set_tuning("device_factor", v)
            assert _lib.get_tuning("device_factor") == v
        for bad in (-1, 3):
            with pytest.raises(_lib.MGXError):
                _lib.set_tuning("device_factor", bad)
        assert _lib.get_tuning("device_factor") == 1
    finally:
        _lib.set_tuning("device_factor", old)

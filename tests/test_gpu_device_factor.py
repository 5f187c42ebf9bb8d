"""Device-pointer uploads factor the velocity on the GPU (tuning key
"device_factor", csrc/vfactor.hip): mgx_upload_device reaches the same factored
passes as mgx_upload.

N=4096, L=7 is the smallest size at which the factors are used.  The host
upload is the reference: the mgx_velocity_factored mask, u, norms, cycle counts
and the cross pass's compulsory bytes (the launch accounting: two fine arrays
fewer with factors, so equality shows without a timer that the fast kernels
ran) must be equal after a device-tensor upload.
"""
import numpy as np
import pytest
import torch   # before libmgx loads: one HIP runtime in the process

from hpcclassmultigridproject_amd import Multigrid, _lib, init_problem

pytestmark = pytest.mark.gpu
NU = -4e-4
N, L = 4096, 7


@pytest.fixture
def knobs():
    """Set tuning keys for one test; restores the previous values."""
    saved = {}

    def set_(**kv):
        for k, v in kv.items():
            saved.setdefault(k, _lib.get_tuning(k))
            _lib.set_tuning(k, v)
    yield set_
    for k, v in saved.items():
        _lib.set_tuning(k, v)


@pytest.fixture(scope="module")
def flow():
    return init_problem(N)


@pytest.fixture(scope="module")
def perturbed(flow):
    u0, v1, v2 = flow
    w = v1.copy()   # not rank-1 any more (tests/test_gpu_vgen.py)
    w[N // 3 * (N + 1) + N // 5] *= 1.0000001
    return u0, w, v2


def _dev(fields):
    return [torch.from_numpy(f).to("cuda") for f in fields]


def _mask(fields, device, tower=_lib.TOWER_REFERENCE, **kw):
    with Multigrid(N, L, 1.0 / N / 10, NU, fp_mode=_lib.FP_FMA, tower_mode=tower, **kw) as mg:
        mg.upload(*(_dev(fields) if device else fields))
        return mg.velocity_factored()


def _run(fields, device, fp, tower=_lib.TOWER_REFERENCE, **kw):
    with Multigrid(N, L, 1.0 / N / 10, NU, fp_mode=fp, tower_mode=tower, **kw) as mg:
        mg.upload(*(_dev(fields) if device else fields))
        fac = mg.velocity_factored()
        mg.rhs()
        if not kw:
            mg.profile(True)
        norms = [mg.run_cycles(1) for _ in range(3)]
        ua = mg.download()
        cyc = [mg.step(1e-6) for _ in range(2)]
        ub = mg.download()
        cb = mg.profile_get_ex(_lib.K_XSMOOTH, 0)[3] if not kw else None
        return fac, norms, ua, cyc, ub, cb


_host = {}


def _host_run(flow, fp, **kw):
    """The host-upload reference, once per configuration."""
    key = (fp, tuple(sorted(kw.items())))
    if key not in _host:
        _host[key] = _run(flow, False, fp, **kw)
    return _host[key]


@pytest.mark.parametrize("tower,want", [(_lib.TOWER_REFERENCE, 7),
                                        (_lib.TOWER_CORRECT, (1 << (L - 1)) - 1)],
                         ids=["reference", "correct"])
def test_device_upload_mask_equals_host_upload(flow, tower, want):
    assert _mask(flow, False, tower) == want
    assert _mask(flow, True, tower) == want


def test_refused_and_switched_off(flow, perturbed, knobs):
    assert _mask(perturbed, True) == 0
    assert _mask(perturbed, True, _lib.TOWER_CORRECT) == 0
    knobs(device_factor=0)
    assert _mask(flow, True) == 0
    assert _mask(flow, False) == 7   # host uploads do not depend on the key's 0 / 1


@pytest.mark.parametrize("fp", [_lib.FP_BITWISE, _lib.FP_FMA], ids=["bitwise", "fma"])
def test_device_upload_outputs_and_traffic(flow, fp):
    fh, nh, uah, ch, ubh, cbh = _host_run(flow, fp)
    fd, nd, uad, cd, ubd, cbd = _run(flow, True, fp)
    assert fd == fh == 7
    assert nd == nh
    assert cd == ch
    assert np.array_equal(uad.view(np.uint64), uah.view(np.uint64))
    assert np.array_equal(ubd.view(np.uint64), ubh.view(np.uint64))
    assert cbh > 0 and cbd == cbh, (cbd, cbh)


def test_device_upload_virtual_ranks(flow):
    fh, nh, uah, ch, ubh, _ = _host_run(flow, _lib.FP_FMA, local_parts=2)
    fd, nd, uad, cd, ubd, _ = _run(flow, True, _lib.FP_FMA, local_parts=2)
    assert fh & 1 and fd == fh, (fd, fh)
    assert cd == ch
    assert np.array_equal(uad.view(np.uint64), uah.view(np.uint64))
    assert np.array_equal(ubd.view(np.uint64), ubh.view(np.uint64))


def test_device_factor_2_host_upload(flow, knobs):
    fh, nh, uah, ch, ubh, cbh = _host_run(flow, _lib.FP_FMA)
    knobs(device_factor=2)
    fd, nd, uad, cd, ubd, cbd = _run(flow, False, _lib.FP_FMA)
    assert fd == fh == 7
    assert nd == nh and cd == ch and cbd == cbh
    assert np.array_equal(uad.view(np.uint64), uah.view(np.uint64))
    assert np.array_equal(ubd.view(np.uint64), ubh.view(np.uint64))

"""mgx_set_velocity / Multigrid.set_velocity: a new velocity on a live context,
the finest u kept in place.

The contract (include/mgx.h): everything that follows is, bit for bit, what a
fresh context gives after mgx_upload(downloaded u, new v1, new v2).  So the
comparison run is always such a fresh context: u as uint64 and cycle counts
equal, norms within 1e-11 relative (the bound mgx.h documents for norms taken
by different kernels).  N=4096, L=7 is the smallest size with velocity
factors; the factor structure changes both ways (mask 7 <-> 0), with and
without captured sub-cycles (graph_level), and at N=128 the CPU oracle pins
that the coarse velocity tower was rebuilt.
"""
import numpy as np
import pytest
import torch   # before libmgx loads: one HIP runtime in the process

from hpcclassmultigridproject_amd import Multigrid, _lib, init_problem

pytestmark = pytest.mark.gpu
NU = -4e-4
N, L = 4096, 7
NORM_RTOL = 1e-11


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
    _, v1, v2 = flow
    w = v1.copy()   # not rank-1 any more (tests/test_gpu_vgen.py)
    w[N // 3 * (N + 1) + N // 5] *= 1.0000001
    return w, v2


def _dev(fields):
    return [torch.from_numpy(f).to("cuda") for f in fields]


def _after(mg):
    """What runs after the velocity changed: V-cycles on a new rhs, then steps."""
    mg.rhs()
    norms = [mg.run_cycles(2)]
    ua = mg.download()
    cyc = [mg.step(1e-6) for _ in range(2)]
    return norms, ua, cyc, mg.download()


def _with_set_velocity(u0, va, vb, fp, tower, device=False):
    with Multigrid(N, L, 1.0 / N / 10, NU, fp_mode=fp, tower_mode=tower) as mg:
        mg.upload(u0, *va)
        ma = mg.velocity_factored()
        cyc0 = [mg.step(1e-6) for _ in range(2)]
        umid = mg.download()
        captures = _lib.get_tuning("graph_captures")
        mg.set_velocity(*(_dev(vb) if device else vb))
        mb = mg.velocity_factored()
        out = _after(mg)
        return ma, mb, cyc0, umid, out, _lib.get_tuning("graph_captures") - captures


def _fresh(umid, vb, fp, tower):
    with Multigrid(N, L, 1.0 / N / 10, NU, fp_mode=fp, tower_mode=tower) as mg:
        mg.upload(umid, *vb)
        return mg.velocity_factored(), _after(mg)


def _same(got, want):
    (ng, uag, cg, ubg), (nw, uaw, cw, ubw) = got, want
    assert cg == cw
    assert np.array_equal(uag.view(np.uint64), uaw.view(np.uint64))
    assert np.array_equal(ubg.view(np.uint64), ubw.view(np.uint64))
    np.testing.assert_allclose(ng, nw, rtol=NORM_RTOL)


@pytest.mark.parametrize("fp,tower", [(_lib.FP_FMA, _lib.TOWER_REFERENCE),
                                      (_lib.FP_FMA, _lib.TOWER_CORRECT),
                                      (_lib.FP_BITWISE, _lib.TOWER_REFERENCE)],
                         ids=["fma-reference", "fma-correct", "bitwise-reference"])
def test_set_velocity_equals_fresh_upload(flow, fp, tower):
    """The reversed flow is still exactly rank-1: the mask is unchanged."""
    u0, v1, v2 = flow
    vb = (-v1, -v2)
    full = 7 if tower == _lib.TOWER_REFERENCE else (1 << (L - 1)) - 1
    ma, mb, _, umid, got, _ = _with_set_velocity(u0, (v1, v2), vb, fp, tower)
    mf, want = _fresh(umid, vb, fp, tower)
    assert ma == mb == mf == full
    assert not np.array_equal(umid, u0)
    _same(got, want)


@pytest.mark.parametrize("tower", [_lib.TOWER_REFERENCE, _lib.TOWER_CORRECT],
                         ids=["reference", "correct"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_factor_structure_changes_both_ways(flow, perturbed, tower, device):
    u0, v1, v2 = flow
    full = 7 if tower == _lib.TOWER_REFERENCE else (1 << (L - 1)) - 1
    for va, vb, masks in (((v1, v2), perturbed, (full, 0)), (perturbed, (v1, v2), (0, full))):
        ma, mb, _, umid, got, _ = _with_set_velocity(u0, va, vb, _lib.FP_FMA, tower, device)
        mf, want = _fresh(umid, vb, _lib.FP_FMA, tower)
        assert (ma, mb) == masks and mf == mb
        _same(got, want)


def test_captured_subcycles_are_dropped(flow, perturbed, knobs):
    """graph_level=3: the captured sub-cycles hold the old velocity's zero
    rows, generator flags and factor pointers, so a new velocity captures
    again; bitwise the uncaptured run."""
    u0, v1, v2 = flow
    knobs(graph_level=0)
    _, _, c0, um0, out0, _ = _with_set_velocity(u0, (v1, v2), perturbed, _lib.FP_FMA,
                                                _lib.TOWER_REFERENCE)
    knobs(graph_level=3)
    ma, mb, c3, um3, out3, captured = _with_set_velocity(u0, (v1, v2), perturbed, _lib.FP_FMA,
                                                         _lib.TOWER_REFERENCE)
    assert (ma, mb) == (7, 0)
    assert captured > 0
    assert c3 == c0
    assert np.array_equal(um3.view(np.uint64), um0.view(np.uint64))
    _same(out3, out0)
    assert out3[0] == out0[0]   # (the same kernels: the norms are equal too)


def test_second_upload_on_a_live_context_with_graphs(flow, perturbed, knobs):
    """A second mgx_upload drops the captured sub-cycles as well."""
    u0, v1, v2 = flow
    out = []
    for g in (0, 3):
        knobs(graph_level=g)
        with Multigrid(N, L, 1.0 / N / 10, NU, fp_mode=_lib.FP_FMA) as mg:
            mg.upload(u0, v1, v2)
            mg.rhs()
            na = mg.run_cycles(2)
            captures = _lib.get_tuning("graph_captures")
            mg.upload(u0, *perturbed)
            assert mg.velocity_factored() == 0
            mg.rhs()
            nb = mg.run_cycles(2)
            out.append((na, nb, mg.download(), _lib.get_tuning("graph_captures") - captures))
    assert out[0][3] == 0 and out[1][3] > 0
    assert out[0][:2] == out[1][:2]
    assert np.array_equal(out[0][2].view(np.uint64), out[1][2].view(np.uint64))


def test_meaning_against_the_cpu_oracle(oracle_mod):
    """Two steps, a random velocity (rng 20220501), two steps == the CPU
    oracle's timestepper run in two legs, the second from the first leg's
    result with the new field: the coarse velocity tower was rebuilt."""
    O = oracle_mod
    n, lv = 128, 3
    dt = 1.0 / n / 10
    u0, v1, v2 = init_problem(n)
    rng = np.random.default_rng(20220501)
    w1 = rng.uniform(-1, 1, v1.size)
    w2 = rng.uniform(-1, 1, v2.size)
    O.set_threads(8)
    ua, ca = O.timestepper(u0, v1, v2, NU, lv, n, dt, 2.5 * dt, 1.0 / n, 1e-6)
    ub, cb = O.timestepper(ua, w1, w2, NU, lv, n, dt, 2.5 * dt, 1.0 / n, 1e-6)
    assert len(ca) == 2 and len(cb) == 2
    with Multigrid(n, lv, dt, NU) as mg:
        mg.upload(u0, v1, v2)
        assert [mg.step(1e-6) for _ in range(2)] == ca
        assert np.array_equal(mg.download().view(np.uint64), ua.view(np.uint64))
        mg.set_velocity(w1, w2)
        assert [mg.step(1e-6) for _ in range(2)] == cb
        got = mg.download()
    assert np.array_equal(got.view(np.uint64), ub.view(np.uint64))
    # (and the old tower would not have given this)
    uc, _ = O.timestepper(ua, v1, v2, NU, lv, n, dt, 2.5 * dt, 1.0 / n, 1e-6)
    assert not np.array_equal(ub, uc)


def test_errors():
    n = 1024
    u0, v1, v2 = init_problem(n)
    with Multigrid(n, 4, 1.0 / n / 10, NU, local_parts=2) as mg:
        mg.upload(u0, v1, v2)
        with pytest.raises(_lib.MGXError) as e:
            mg.set_velocity(v1, v2)
        assert e.value.code == _lib.MGX_E_ARG
        assert "partitioned" in str(e.value)
    with Multigrid(n, 4, 1.0 / n / 10, NU) as mg:
        mg.upload(u0, v1, v2)
        lib = _lib.lib()
        assert lib.mgx_set_velocity(mg.handle, None, v2.ctypes.data) == _lib.MGX_E_ARG
        assert lib.mgx_set_velocity(mg.handle, v1.ctypes.data, None) == _lib.MGX_E_ARG
        assert lib.mgx_set_velocity_device(mg.handle, None, None) == _lib.MGX_E_ARG
        mg.set_velocity(v1, v2)   # and the context still works
        mg.rhs()
        assert mg.run_cycles(1) > 0

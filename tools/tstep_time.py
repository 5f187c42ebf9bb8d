"""DESIGN.md section 12's measurements of mgx_set_time_step on one GPU.
    python tools/tstep_time.py [--N 16384 --L 9 --steps 10 --samples 5 --out FILE.json]

Steps (section 9 / 11's protocol: HIP events on the context's stream around
`steps` steps, one context per variant, all alive in one process, the variants
interleaved, `samples` samples after one warm-up sample; median, min, max in ms
per step):
  default        mgx_step, nothing set
  new_dt         mgx_set_time_step with a new dt before every step, theta = 1/2
  theta1         theta = 1 (set once)
  theta1_source  theta = 1 with a one-term separable source
The first pass alone (profile kind MGX_K_RHS, finest level, HIP events around
each launch; u never changes: tol = 2 ends mg_outer before its first cycle):
  pass2          the two-operator pass (theta = 1; init_problem's velocity has
                 factors, which the pass reads: 16 B per point)
  pass2_2d       the same with source_sv 0: the 2-D v1 / v2 (32 B per point)
  fused          the rhs + norm pass of theta = 1/2 (step_fuse / step_cross 0)
  two_launch     mgx_rhs + mgx_residual_norm(0) (theta = 1), the sum
"""
import argparse
import ctypes as C
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, '.')
import hpcclassmultigridproject_amd as pkg
from hpcclassmultigridproject_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument('--N', type=int, default=16384)
ap.add_argument('--L', type=int, default=9)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--samples', type=int, default=5)
ap.add_argument('--tol', type=float, default=1e-6)
ap.add_argument('--out', default='')
a = ap.parse_args()
N, L = a.N, a.L
dt, nu = 1.0 / N / 10, -4e-4

hip = C.CDLL('libamdhip64.so')


def hipchk(rc):
    if rc != 0:
        raise RuntimeError(f"hip error {rc}")


class Timer:
    """Two HIP events on a context's stream."""

    def __init__(self, mg):
        self.s = C.c_void_p(mg.stream())
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        hipchk(hip.hipEventCreate(C.byref(self.e0)))
        hipchk(hip.hipEventCreate(C.byref(self.e1)))

    def start(self):
        hipchk(hip.hipEventRecord(self.e0, self.s))

    def stop(self):
        hipchk(hip.hipEventRecord(self.e1, self.s))
        hipchk(hip.hipEventSynchronize(self.e1))
        ms = C.c_float()
        hipchk(hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1))
        return ms.value


def stat(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


u0, v1, v2 = pkg.init_problem(N, nthreads=16)
x = np.arange(N + 1) / N
sa, sb = 8.0 * np.exp(-40 * (x - .35) ** 2), 1.0 + .5 * np.cos(5 * x)


def make(theta=None, source=False):
    mg = pkg.Multigrid(N, L, dt, nu, device=0, fp_mode=_lib.FP_FMA)
    mg.upload(u0, v1, v2)
    if source:
        mg.set_source_separable(sa, sb)
    if theta is not None:
        mg.set_time_step(dt, theta)
    return mg


def plain(mg, k):
    return mg.step(a.tol)


def new_dt(mg, k):
    mg.set_time_step(dt * (1.0 + 1e-3 * (k & 1)), .5)
    return mg.step(a.tol)


variants = [("default", make(), plain), ("new_dt", make(), new_dt),
            ("theta1", make(1.0), plain), ("theta1_source", make(1.0, True), plain)]
timers = {name: Timer(mg) for name, mg, _ in variants}
ms = {name: [] for name, _, _ in variants}
cycles = {name: [] for name, _, _ in variants}
for sample in range(a.samples + 1):   # (the first is the warm-up)
    for name, mg, step in variants:
        mg.synchronize()
        timers[name].start()
        cyc = [step(mg, k) for k in range(a.steps)]
        t = timers[name].stop() / a.steps
        if sample:
            ms[name].append(t)
            cycles[name].append(cyc)
result = {"N": N, "L": L, "steps": a.steps, "samples": a.samples, "tol": a.tol,
          "build": _lib.build_id(), "ms_per_step": {}, "pass_ms": {}}
for name, _, _ in variants:
    result["ms_per_step"][name] = dict(stat(ms[name]), cycles=cycles[name][-1])
    print(name, result["ms_per_step"][name], flush=True)
for _, mg, _ in variants:
    mg.close()

# ---- the first pass alone
mg = make()
mg.profile(True, finest_only=True)
saved = {k: _lib.get_tuning(k) for k in ("step_fuse", "step_cross")}


def kind_ms(kinds):
    out = 0.0
    for kd in kinds:
        n, t, _ = mg.profile_get(kd, 0)
        out += t / n
    mg.profile_reset()
    return out


def run_pass2():
    mg.set_time_step(dt, 1.0)
    for _ in range(5):
        mg.step_ex(2.0)
    return kind_ms([_lib.K_RHS])


def run_fused():
    mg.set_time_step(dt, .5)
    for k in saved:
        _lib.set_tuning(k, 0)
    try:
        for _ in range(5):
            mg.step_ex(2.0)
    finally:
        for k, v in saved.items():
            _lib.set_tuning(k, v)
    return kind_ms([_lib.K_RHS])


def run_two():
    mg.set_time_step(dt, 1.0)
    for _ in range(5):
        mg.rhs()
        mg.residual_norm(0)
    return kind_ms([_lib.K_RHS, _lib.K_RESNORM])


def run_pass2_2d():
    sv = _lib.get_tuning("source_sv")
    _lib.set_tuning("source_sv", 0)
    try:
        return run_pass2()
    finally:
        _lib.set_tuning("source_sv", sv)


passes = [("pass2", run_pass2), ("pass2_2d", run_pass2_2d), ("fused", run_fused),
          ("two_launch", run_two)]
pms = {name: [] for name, _ in passes}
for sample in range(a.samples + 1):
    for name, fn in passes:
        mg.profile_reset()
        t = fn()
        if sample:
            pms[name].append(t)
for name, _ in passes:
    result["pass_ms"][name] = stat(pms[name])
    print(name, result["pass_ms"][name], flush=True)
mg.close()
if a.out:
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)

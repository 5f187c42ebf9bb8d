"""xpack = 0 / 1 / 2 alternated on one context (N=16384, L=9, fma): ms per time
step (4 steps of mg_outer to 1e-6) and ms per cycle of run_cycles(10); u bitwise.
    python tools/ab_xpack_step.py"""
import sys, time
sys.path.insert(0, '.')
import numpy as np
import hpcclassmultigridproject_amd as pkg
from hpcclassmultigridproject_amd import _lib
N, L = 16384, 9
u0, v1, v2 = pkg.init_problem(N, nthreads=16)
mg = pkg.Multigrid(N, L, 1.0 / N / 10, -4e-4, device=0, fp_mode=_lib.FP_FMA)
ref = None
for rnd in range(3):
    for xp in (0, 1, 2):
        _lib.set_tuning("xpack", xp)
        mg.upload(u0, v1, v2)
        mg.step(1e-6); mg.synchronize()
        t = time.perf_counter(); cyc = [mg.step(1e-6) for _ in range(4)]; mg.synchronize()
        ms = (time.perf_counter() - t) / 4 * 1e3
        t = time.perf_counter(); mg.run_cycles(10); mg.synchronize()
        rc = (time.perf_counter() - t) / 10 * 1e3
        print(f"round {rnd} xpack={xp}: step {ms:.3f} ms (cycles {cyc}), run_cycles(10) {rc:.3f} ms/cycle", flush=True)
        if rnd == 0:
            u = mg.download()
            if ref is None: ref = u
            else: print("   u bitwise vs xpack=0:", bool(np.array_equal(u, ref)), flush=True)
mg.close()

"""the BDF2 pass against its alternatives, and ms per step with and
without a history.  One process, one context, the variants alternated.

    python tools/bdf_time.py [--n 16384] [--levels 9] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

import hpcclassmultigridproject_amd as pkg   # noqa: E402
from hpcclassmultigridproject_amd import _lib   # noqa: E402

NU, TOL = -4e-4, 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--levels", type=int, default=9)
    ap.add_argument("--samples", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, L = a.n, a.levels
    dt = 1.0 / N / 10
    u0, v1, v2 = pkg.init_problem(N)
    out = {"N": N, "L": L}
    with pkg.Multigrid(N, L, dt, NU, fp_mode=_lib.FP_FMA, device=0) as mg:
        mg.upload(u0, v1, v2)
        out["velocity_factored"] = mg.velocity_factored()
        mg.set_history()

        def launch_ms(fn, kind):
            mg.profile_reset()
            mg.profile(True, finest_only=True)
            fn()
            mg.synchronize()
            n, ms, _, _ = mg.profile_get_ex(kind, 0)
            mg.profile(False)
            return ms / n
        for _ in range(3):   # warm-up: both kinds of step
            mg.step(TOL)
            mg.step_bdf2(TOL)
        pitch = (N + 1 + 15) // 16 * 16
        src = torch.empty((N + 1) * pitch, dtype=torch.float64, device="cuda")
        dst = torch.empty_like(src)
        rows = {"bdf_pass": [], "rhs": [], "resnorm": [], "copy": [], "theta_pass": []}
        for _ in range(a.samples):
            mg.set_time_step(dt, .5)
            mg.step(TOL)
            rows["bdf_pass"].append(launch_ms(lambda: mg.step_bdf2(TOL), _lib.K_RHS))
            rows["rhs"].append(launch_ms(mg.rhs, _lib.K_RHS))
            rows["resnorm"].append(launch_ms(lambda: mg.residual_norm(0), _lib.K_RESNORM))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            rows["copy"].append(e0.elapsed_time(e1))
            mg.set_time_step(dt, .75)
            rows["theta_pass"].append(launch_ms(lambda: mg.step_ex(TOL), _lib.K_RHS))
        out["pass_ms"] = rows
        out["pass_ms_median"] = {k: float(np.median(v[1:])) for k, v in rows.items()}

        def steps(fn, n=10):
            ts, cyc = [], []
            for _ in range(n):
                mg.synchronize()
                t0 = time.perf_counter()
                c = fn()
                mg.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                cyc.append(c if isinstance(c, int) else c[0])
            return {"median": float(np.median(ts[2:])), "all": ts, "cycles": cyc}
        mg.set_time_step(dt, .5)
        mg.step(TOL)
        out["step_ms_bdf2"] = steps(lambda: mg.step_bdf2(TOL))
        out["step_ms_theta_history"] = steps(lambda: mg.step(TOL))
        mg.set_history(False)
        mg.step(TOL)
        out["step_ms_theta_no_history"] = steps(lambda: mg.step(TOL))
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

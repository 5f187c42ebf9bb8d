"""the step error pass beside stats("u", minus=...), and ms per BDF2
step at a history depth.

    python tools/errest_time.py pass [--n 16384] [--levels 9] [--out FILE.json]
    python tools/errest_time.py step --depth 2 [--pkg-root DIR] [--out FILE.json]

pass: one context at depth 2 after two steps; the two reduction passes
alternated in one process, device time from the read-only keys errest_us /
stats_us (HIP events around the launches), one warm-up sample, then --samples.
step: host clock around 10 synchronised mgx_step_bdf2 calls, one warm-up
sample, then --samples; --depth 1 uses mgx_set_history alone, so with
--pkg-root it also runs on a checkout that has no depth 2 (the parent commit).
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["pass", "step"])
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--levels", type=int, default=9)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--depth", type=int, default=2, choices=[1, 2])
    ap.add_argument("--pkg-root", default=os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg_root))
    import numpy as np
    import torch
    import hpcclassmultigridproject_amd as pkg
    from hpcclassmultigridproject_amd import _lib

    N, L = a.n, a.levels
    NU, TOL = -4e-4, 1e-6
    dt = 1.0 / N / 10
    u0, v1, v2 = pkg.init_problem(N)
    out = {"mode": a.mode, "N": N, "L": L, "build": _lib.build_id()}

    def spread(xs):
        return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)),
                "all": [float(x) for x in xs]}
    with pkg.Multigrid(N, L, dt, NU, fp_mode=_lib.FP_FMA, device=0) as mg:
        mg.upload(u0, v1, v2)
        if a.mode == "pass":
            mg.set_history_depth(2)
            mg.step(TOL)
            mg.step_bdf2(TOL)
            minus = torch.from_numpy(mg.sample(1, "history")).cuda().ravel()
            err_us, st_us = [], []
            for k in range(a.samples + 1):
                rec = mg.step_error(1e-6, 1e-3)
                e = _lib.get_tuning("errest_us")
                st = mg.stats("u", interior=True, minus=minus)
                s = _lib.get_tuning("stats_us")
                if k:   # (the first sample warms up)
                    err_us.append(e)
                    st_us.append(s)
            eb, sb = _lib.get_tuning("errest_bytes"), _lib.get_tuning("stats_bytes")
            out["errest_us"], out["stats_minus_us"] = spread(err_us), spread(st_us)
            out["errest_bytes"], out["stats_minus_bytes"] = eb, sb
            out["errest_GBps"] = eb / np.median(err_us) * 1e-3
            out["stats_minus_GBps"] = sb / np.median(st_us) * 1e-3
            out["record"] = {f: getattr(rec, f) for f in rec.FIELDS}
            out["record"]["rms"] = rec.rms
            out["c_max_against_stats"] = [rec.c_max, max(abs(st.min), abs(st.max))]
        else:
            out["depth"] = a.depth
            if a.depth == 2:
                mg.set_history_depth(2)
            else:
                mg.set_history()
            mg.step(TOL)
            ms, cycles = [], []
            for k in range(a.samples + 1):
                mg.synchronize()
                t0 = time.perf_counter()
                cyc = [mg.step_bdf2(TOL)[0] for _ in range(10)]
                mg.synchronize()
                if k:
                    ms.append((time.perf_counter() - t0) * 1e2)   # ms per step
                    cycles.append(cyc)
            out["bdf2_step_ms"] = spread(ms)
            out["cycles"] = cycles
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""the dense output passes at N=16384 after two BDF2 steps.

    python tools/dense_time.py [--n 16384] [--levels 9] [--samples 5] [--out FILE.json]

One context at depth 2 (a theta-step and two BDF2 steps), one process.  Device
time from the read-only keys dense_us / errest_us (HIP events around the
launches), one warm-up sample, then --samples of every variant in turn:

  march     mg.dense(order, tau, out=device tensor) for orders 0..2 in the row
            groups of the error pass ("dense_rows" 0), with plain ("dense_store"
            0), non-temporal (1) and 8-byte-aligned 16-byte (2) stores alternated
  rows      the same with 1, 2, 4, 8 and 16 rows per workgroup ("dense_rows";
            4 is the default), stores 0 and 2
  errest    mg.step_error, the same frame with three reads and no write
  stream    mgx_stream_bandwidth with nin = 4
  old       the route without the pass: `levels` device copies (mgx_sample_device
            at stride 1) and the combination in torch, host clock around
            synchronised calls
  stride64, points1024   the gather and 1024 probes at order 2
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--levels", type=int, default=9)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    import hpcclassmultigridproject_amd as pkg
    from hpcclassmultigridproject_amd import _lib

    N, L = a.n, a.levels
    NU, TOL = -4e-4, 1e-6
    dt = 1.0 / N / 10
    u0, v1, v2 = pkg.init_problem(N)
    out = {"N": N, "L": L, "build": _lib.build_id()}

    def spread(xs):
        return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)),
                "all": [float(x) for x in xs]}
    cnt = (N + 1) ** 2
    with pkg.Multigrid(N, L, dt, NU, fp_mode=_lib.FP_FMA, device=0) as mg:
        mg.upload(u0, v1, v2)
        mg.set_history_depth(2)
        mg.step(TOL)
        mg.step_bdf2(TOL)
        mg.step_bdf2(TOL)
        tau = -dt / 3
        dst = torch.empty(cnt, dtype=torch.float64, device="cuda:0")
        tmp = [torch.empty(cnt, dtype=torch.float64, device="cuda:0") for _ in range(3)]
        w = pkg.dense_weights(2, tau, dt, dt)
        rng = np.random.default_rng(15)
        pi = torch.from_numpy(rng.integers(0, N + 1, 1024)).cuda()
        pj = torch.from_numpy(rng.integers(0, N + 1, 1024)).cuda()
        pic = torch.empty((N // 64 + 1) ** 2, dtype=torch.float64, device="cuda:0")
        us = {}

        def rec(key, v):
            us.setdefault(key, []).append(v)
        fields = ("u", "history", "history2")
        rows0 = _lib.get_tuning("dense_rows")   # the default; "march" below uses 0, the frame
        out["dense_rows_default"] = rows0
        for k in range(a.samples + 1):
            _lib.set_tuning("dense_rows", 0)
            for order in (0, 1, 2):
                for nt in (0, 1, 2):
                    _lib.set_tuning("dense_store", nt)
                    mg.dense(order, tau, out=dst)
                    rec(f"march_order{order}_nt{nt}", _lib.get_tuning("dense_us"))
                    out[f"march_order{order}_bytes"] = _lib.get_tuning("dense_bytes")
            _lib.set_tuning("dense_store", 0)
            for rows in (1, 2, 4, 8, 16):   # the rows of a workgroup ("dense_rows")
                for order in (0, 1, 2):
                    for st in (0, 2):
                        _lib.set_tuning("dense_rows", rows)
                        _lib.set_tuning("dense_store", st)
                        mg.dense(order, tau, out=dst)
                        rec(f"march_order{order}_st{st}_rows{rows}", _lib.get_tuning("dense_us"))
            _lib.set_tuning("dense_rows", rows0)
            _lib.set_tuning("dense_store", 0)
            mg.step_error(1e-6, 1e-3)
            rec("errest", _lib.get_tuning("errest_us"))
            out["errest_bytes"] = _lib.get_tuning("errest_bytes")
            mg.dense(2, tau, stride=64, out=pic)
            rec("stride64_order2", _lib.get_tuning("dense_us"))
            mg.dense_points(2, tau, pi, pj)
            rec("points1024_order2", _lib.get_tuning("dense_us"))
            for levels in (1, 2, 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for f in range(levels):
                    mg.sample(1, fields[f], out=tmp[f])
                if levels == 1:
                    res = tmp[0]
                elif levels == 2:
                    res = w[0] * tmp[0] + w[1] * tmp[1]
                else:
                    res = w[0] * tmp[0] + w[1] * tmp[1] + w[2] * tmp[2]
                torch.cuda.synchronize()
                rec(f"old_route_levels{levels}", (time.perf_counter() - t0) * 1e6)
                del res
        for key in list(us):
            us[key] = spread(us[key][1:])   # (the first sample warms up)
        out["us"] = us
        for order in (0, 1, 2):
            for nt in (0, 1, 2):
                out[f"march_order{order}_nt{nt}_GBps"] = \
                    out[f"march_order{order}_bytes"] / us[f"march_order{order}_nt{nt}"]["median"] * 1e-3
        out["errest_GBps"] = out["errest_bytes"] / us["errest"]["median"] * 1e-3
    bw = [_lib.stream_bandwidth(1 << 30, 4, 10) for _ in range(3)]
    out["stream_nin4_GBps"] = spread(bw)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

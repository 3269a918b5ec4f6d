#!/usr/bin/env python3
"""Per-stage wall-clock of MPLS (Algorithms/MPLS.m) on bench.generate's C2 / C4 problems, synchronised host clock.

Stages of one desc_mpls_run_dev call (desc_mpls_info: CEMP, MST, loop, total), then the loop's pieces measured one by one on the
same device problem: the stand-alone MST (desc_mst_run_dev) and, per MPLS iteration, Weighted_LAA + residuals + H step + quantile
taken from a run with max_iter = 2 (one iteration) minus the initialisation-only run (max_iter = 1).

    python tools/mpls_stages.py [--configs C2,C4] [--reps 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from desc_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C4")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    beta_c = [2.0 ** k for k in range(6)]
    tau = [0.95, 0.9, 0.85, 0.8]
    alpha = 1.0 / (np.arange(1, 101) + 1)
    for name in a.configs.split(","):
        mo, nn, ii, jj, rij = bench.generate(name)
        prob = _lib.ProblemArrays(nn, ii, jj, rij)
        dp = _lib.DeviceProblem(prob, 0)
        try:
            run = lambda max_iter: _lib.mpls_run(dp, beta_c, 6, 50, 1e-3, max_iter, [32.0], tau, alpha)   # noqa: E731
            run(100)                                                                   # warm-up (code objects, block cache)
            rows = []
            for _ in range(a.reps):
                _, _, S, info = run(100)
                t0 = time.perf_counter(); _lib.mst_run(dp, S); t_mst = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter(); run(1); t1 = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter(); run(2); t2 = (time.perf_counter() - t0) * 1e3
                rows.append((info, t_mst, t2 - t1))
            info = rows[-1][0]
            med = lambda k: float(np.median([r[0][k] for r in rows]))                  # noqa: E731
            print(f"{name}: n={nn} m={prob.m} m_pos={info['m_pos']} iterations={info['iters']} cg_iters={info['cg_iters']}")
            print(f"  desc_mpls_run_dev   total {med('ms_total'):9.2f} ms   CEMP {med('ms_cemp'):8.2f}   MST {med('ms_mst'):7.2f}   "
                  f"loop {med('ms_loop'):8.2f}  ({med('ms_loop') / max(info['iters'], 1):.2f} ms per iteration incl. set-up)")
            print(f"  desc_mst_run_dev    {np.median([r[1] for r in rows]):8.2f} ms (upload of SVec included)")
            print(f"  one MPLS iteration  {np.median([r[2] for r in rows]):8.2f} ms (Weighted_LAA + residuals + H step + quantile + weights)")
        finally:
            dp.free()


if __name__ == "__main__":
    main()

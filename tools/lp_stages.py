#!/usr/bin/env python3
"""Per-stage times of linprog_sij (Algorithms/linprog_sij.m) on bench.generate's C2 / C4 problems.

One full call per configuration on a resident device problem: samples + S0Mat, the transposed incidence, the PDHG loop to `tol`
(desc_lp_info, synchronised host clock), then the weighted spectral step and the refinement.  The loop's two kernels are timed in a
second, short run with hipEvent laps around each launch (verbose = 2: every step synchronises, so that run's total is not a loop time).
Bytes are counted from the arrays each kernel touches, a gathered double as
8 bytes: per cycle the row kernel reads two indices (8), S0 (8), y (16), the running sum of y (16) and two gathered xbar (16) and writes
y (16), the sum (16) and z (8) = 104 B; the column kernel reads per cycle two list entries (8) and two gathered z (16) = 24 B, and per
edge 72 B of x, xbar, own, tau, list bounds and the running sum.  The fraction is against the 6.29 TB/s copy rate DESIGN.md uses.

    python tools/lp_stages.py [--configs C2,C4] [--max-iter N] [--tol 1e-4] [--out-dir profiles --tag r07]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from desc_amd import _lib  # noqa: E402
from desc_amd.algorithms import Rotation_Alignment  # noqa: E402

COPY_RATE = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C4")
    ap.add_argument("--max-iter", type=int, default=0, help="0: the library's default")
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--lap-steps", type=int, default=192)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--verbose", action="store_true", help="one line per check of the full solve")
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--tag", default="lp")
    a = ap.parse_args()
    for name in a.configs.split(","):
        mo, nn, ii, jj, rij = bench.generate(name)
        prob = _lib.ProblemArrays(nn, ii, jj, rij)
        dp = _lib.DeviceProblem(prob, 0)
        try:
            p = _lib.default_lp_params()
            p.seed = a.seed; p.tol = a.tol
            q = _lib.LpParams.from_buffer_copy(p)
            q.max_iter = 64
            _lib.lp_sij_run(dp, q, want_k=False)                                        # warm-up (code objects, block cache)
            if a.max_iter:
                p.max_iter = a.max_iter
            p.verbose = 1 if a.verbose else 0
            S, _, _, lp = _lib.lp_sij_run(dp, p, want_k=False)
            q.max_iter = a.lap_steps; q.verbose = 2; q.tol = 0.0
            _, _, _, laps = _lib.lp_sij_run(dp, q, want_k=False)
            R_gcw, sinfo = _lib.spectral_run(dp, np.exp(-5.0 * S), True)
            Rest, rinfo = _lib.refine_run(dp, S, R_gcw, 1e-3, 200)
        finally:
            dp.free()
        mc = lp["rows"] // 2
        b_row = 104.0 * mc
        b_col = 24.0 * mc + 72.0 * lp["m_pos"]
        rec = dict(config=name, n=int(nn), m=int(prob.m), m_pos=int(lp["m_pos"]), nsample=int(lp["nsample"]), rows=int(lp["rows"]), tol=a.tol,
                   max_iter=int(p.max_iter), iters=int(lp["iters"]), restarts=int(lp["restarts"]), converged=int(lp["converged"]),
                   viol=lp["viol"], pobj=lp["pobj"], dobj=lp["dobj"], rel_gap=(lp["pobj"] - lp["dobj"]) / (1 + abs(lp["pobj"]) + abs(lp["dobj"])),
                   ms_samples_s0=lp["ms_samples"], ms_transpose=lp["ms_transpose"], ms_loop=lp["ms_loop"],
                   ms_per_iter_loop=lp["ms_loop"] / max(lp["iters"], 1), lap_steps=int(laps["iters"]),
                   ms_col_kernel=laps["ms_col"], ms_row_kernel=laps["ms_row"], bytes_col_kernel=b_col, bytes_row_kernel=b_row,
                   col_fraction_of_copy_rate=b_col / (laps["ms_col"] * 1e-3) / COPY_RATE if laps["ms_col"] > 0 else None,
                   row_fraction_of_copy_rate=b_row / (laps["ms_row"] * 1e-3) / COPY_RATE if laps["ms_row"] > 0 else None,
                   ms_spectral=sinfo["ms_total"], ms_refine=rinfo["ms_total"], refine_iters=int(rinfo["iters"]), cg_unconverged=int(rinfo["cg_unconverged"]),
                   mean_abs_S_minus_ErrVec=float(np.abs(S - mo.ErrVec).mean()),
                   rot_err_deg_R_gcw=list(Rotation_Alignment(R_gcw, mo.R_orig)[2:]), rot_err_deg_Rest=list(Rotation_Alignment(Rest, mo.R_orig)[2:]))
        print(json.dumps(rec), flush=True)
        if a.out_dir:
            with open(os.path.join(a.out_dir, f"{a.tag}_lp_{name.lower()}.json"), "w") as f:
                json.dump(rec, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Per-stage wall-clock of IRLS_GM / IRLS_L12 (Algorithms/IRLS_GM.m, IRLS_L12.m) on bench.generate's C2 / C4 problems.

One desc_irls_run_dev call per mode on a resident device problem; the stages are desc_irls_info's (projection, components, tree
start, L1 stage and the PCG part of it, IRLS stage, total), with the CG steps per batched Newton solve (one CG for the three
coordinates; each solve's count is rounded up to the probe interval 5) and per IRLS step (laa_step goes through the same PCG,
laa_pcg in csrc/laa.hip, and probes every 25 steps, so that
figure is an upper bound in steps of 25), and the mean / median rotation error after Rotation_Alignment.

    python tools/irls_stages.py [--configs C2,C4] [--modes GM,L12] [--reps 2]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from desc_amd import Rotation_Alignment, _lib  # noqa: E402
from desc_amd.algorithms import marshal_edges  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C4")
    ap.add_argument("--modes", default="GM,L12")
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    keys = ("ms_project", "ms_components", "ms_tree", "ms_l1", "ms_l1_pcg", "ms_irls", "ms_total")
    for name in a.configs.split(","):
        mo = bench.generate(name)[0]
        n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
        prob = _lib.ProblemArrays(n, ii, jj, rij)
        dprob = _lib.DeviceProblem(prob, 0)
        try:
            for mode in a.modes.split(","):
                code = _lib.IRLS_GM if mode == "GM" else _lib.IRLS_L12
                best = None
                for _ in range(a.reps):
                    R, R1, info = _lib.irls_run(dprob, code, order=perm)
                    if best is None or info["ms_total"] < best[2]["ms_total"]:
                        best = (R, R1, info)
                R, R1, info = best
                _, _, me, md = Rotation_Alignment(R, mo.R_orig)
                _, _, me1, md1 = Rotation_Alignment(R1, mo.R_orig)
                print(f"{name} n={n} m={ii.size} {mode}: " + " ".join(f"{k[3:]}={info[k]:.1f}" for k in keys) +
                      f" | L1 iters {info['l1_iters']} PD steps {info['pd_steps']} Newton solves {info['pd_solves']}"
                      f" CG/solve {info['cg_iters_l1'] / max(info['pd_solves'], 1):.1f} (probe 5)"
                      f" | IRLS iters {info['irls_iters']} CG/IRLS-step {info['cg_iters_irls'] / max(info['irls_iters'], 1):.1f} (probe 25)"
                      f" | ill {info['pd_ill']} stuck {info['pd_stuck']} cg_unconverged {info['cg_unconverged']}"
                      f" | err mean/median L1 {me1:.4f}/{md1:.4f} final {me:.4f}/{md:.4f} deg", flush=True)
        finally:
            dprob.free()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The reference's demo (Demo/compare_algorithms.m:9-99) through the Python mirror of its MATLAB calls, on the GPU.

Same model (Uniform_Topology n, p, q, sigma, 'uniform'; the demo's defaults n = 100 ... BASELINE configs[0] uses n = 200), same
parameter structs (:25-46), same calls in the same order, rotations aligned with Rotation_Alignment (:75-82) and tabulated (:85-99).
The default table has four rows: Spectral, CEMP+GCW (the composition CEMP() -> GCW()), DESC_init and DESC.  ``--full`` /
``run(full=True)`` adds the demo's MPLS call (:59) with its MPLS_parameters (:32-36) -- the rows CEMP+MST and MPLS -- and takes
CEMP+GCW from the reference's own CEMP_GCW() (weights 1/(SVec + 1e-8), CEMP_GCW.m:144): six rows.  ``--irls`` / ``run(irls=True)``
adds the demo's IRLS_GM and IRLS_L12 calls (:68-69) -- the rows IRLS-GM and IRLS-L0.5; with both switches the table has the demo's
eight rows in its order (:88-99).  ``--lp`` / ``run(lp=True)`` appends an LP row: linprog_sij() (Algorithms/linprog_sij.m, which the demo
does not call) on the same model.

    python examples/compare_algorithms.py [--n 200] [--p 0.5] [--q 0.2] [--sigma 0.1] [--seed 0] [--full] [--irls] [--lp]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from desc_amd import (CEMP, CEMP_GCW, DESC, GCW, IRLS_GM, IRLS_L12, MPLS, ConstantStepSize, Rotation_Alignment, Spectral,  # noqa: E402
                      Uniform_Topology, linprog_sij)


def run(n=200, p=0.5, q=0.2, sigma=0.1, seed=0, verbose=True, full=False, irls=False, lp=False):
    model_out = Uniform_Topology(n, p, q, sigma, "uniform", seed=seed)                  # :13
    Ind, RijMat, ErrVec, R_orig = model_out.Ind, model_out.RijMat, model_out.ErrVec, model_out.R_orig   # :20-23
    CEMP_parameters = dict(max_iter=6, reweighting=[2.0 ** k for k in range(6)], nsample=50, gcw_beta=5)   # :26-29
    lr = 0.01                                                                            # :38-46
    DESC_parameters = dict(iters=100, learning_rate=lr, make_plots=False, Gradient=ConstantStepSize(lr), R_orig=R_orig, ErrVec=ErrVec,
                           verbose=verbose)
    R_SP = Spectral(Ind, RijMat)                                                         # :63
    SVec = CEMP(Ind, RijMat, CEMP_parameters)                                            # :66 (CEMP_GCW.m = CEMP.m + GCW.m)
    R_CEMP_GCW = GCW(Ind, None, RijMat, SVec)
    R_DESC, R_DESC_init, S_vec = DESC(Ind, RijMat, DESC_parameters)                      # :72
    table = [("Spectral", R_SP), ("CEMP+GCW", R_CEMP_GCW), ("DESC_init", R_DESC_init), ("DESC", R_DESC)]
    if full:
        MPLS_parameters = dict(stop_threshold=1e-3, max_iter=100, reweighting=CEMP_parameters["reweighting"][-1],      # :32-36
                               thresholding=[0.95, 0.9, 0.85, 0.8], cycle_info_ratio=1.0 / (np.arange(1, 101) + 1))
        R_MPLS, R_CEMP_MST = MPLS(Ind, RijMat, dict(CEMP_parameters, verbose=verbose), MPLS_parameters)               # :59
        R_CEMP_GCW_ref = CEMP_GCW(Ind, RijMat, CEMP_parameters)                                                      # :66
        table[1:2] = [("CEMP+MST", R_CEMP_MST), ("CEMP+GCW", R_CEMP_GCW_ref), ("MPLS", R_MPLS)]                      # the demo's six rows (:88-95)
    if irls:
        R_IRLS_GM = IRLS_GM(RijMat, Ind)                                                 # :68
        R_IRLS_L12 = IRLS_L12(RijMat, Ind)                                               # :69
        table[1:1] = [("IRLS-GM", R_IRLS_GM), ("IRLS-L0.5", R_IRLS_L12)]                 # :90-91
    extra = {}
    if lp:
        R_LP, S_lp = linprog_sij(Ind, RijMat, dict(seed=seed, verbose=verbose))
        table.append(("LP", R_LP))
        extra["mean_abs_err_lp"] = float(abs(S_lp - ErrVec).mean())
    rows = []
    for name, R in table:
        _, _, mean_error, median_error = Rotation_Alignment(R, R_orig)                   # :75-82
        rows.append((name, float(mean_error), float(median_error)))
    return rows, dict(extra, mean_abs_err_cemp=float(abs(SVec - ErrVec).mean()), mean_abs_err_desc=float(abs(S_vec - ErrVec).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200); ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--q", type=float, default=0.2); ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0); ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--full", action="store_true", help="add the CEMP+MST, MPLS and reference CEMP+GCW rows")
    ap.add_argument("--irls", action="store_true", help="add the IRLS-GM and IRLS-L0.5 rows")
    ap.add_argument("--lp", action="store_true", help="add the LP row (linprog_sij)")
    a = ap.parse_args()
    rows, extra = run(a.n, a.p, a.q, a.sigma, a.seed, verbose=not a.quiet, full=a.full, irls=a.irls, lp=a.lp)
    print("\nResults =\n")                                                              # :85-99
    print("    %-16s %-12s %-12s" % ("Algorithms", "MeanError", "MedianError"))
    for name, me, md in rows:
        print("    %-16s %-12.4f %-12.4f" % ('"' + name + '"', me, md))
    print("\n(degrees; corruption levels: mean |SVec - ErrVec| CEMP %.4f, DESC %.4f%s)"
          % (extra["mean_abs_err_cemp"], extra["mean_abs_err_desc"], ", LP %.4f" % extra["mean_abs_err_lp"] if a.lp else ""))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A small Monte-Carlo study in ONE batched call: mean |S_vec - ErrVec| against the corruption level q, averaged over a few trials
of Uniform_Topology(100, 0.5, q, 0.1) -- the shape of the figures the DESC paper draws (error against q on graphs of 100-200 nodes).

    python examples/monte_carlo.py [--trials 5] [--n 100] [--iters 100] [--build host|device] [--rotations] [--refined] [--baselines]
                                   [--mpls] [--lp] [--irls] [--device-models] [--resident] [--eig lds|streamed|auto]

--device-models: the trials are drawn on the GPU by one Uniform_Topology_batch call instead of one Uniform_Topology call per trial on the
host.  The batched generator has streams of its own: the curves differ from an unflagged run in their draws, not in their distribution.
The time the generation took is printed in both modes.

--resident: the trials become ONE ProblemBatch -- validated, laid out and uploaded once -- and every selected curve runs on it: with
--device-models the generator hands its problems over on the device (no rotation is copied back before a curve asks for it), otherwise
the host-drawn trials are wrapped.  The DESC, CEMP, MST, MPLS and IRLS curves create their handles on the set; the LP curve reads its
host mirror.  The curves are the same to the last bit as without the flag.

--build: the builder of the cycle structures behind DESC_PGD_batch / DESC_init_batch / DESC_batch: per problem on host threads (the
default) or for the whole batch on the device; the curves are the same to the last bit.

--eig: where the batched eigen-solve behind --rotations, --refined, --baselines (CEMP+GCW) and --lp keeps its blocks.  The default
"lds" takes problems of up to 278 nodes; "auto" solves larger ones with the streamed kernel, so that e.g. --n 400 --refined runs
(DESC_batch and the LP row then take up to 748 nodes, the refinement's cap).  The curves of a size both kernels take are the same to
the last bit.

--rotations: the demo's own metric next to it -- one DESC_init_batch call (the PGD pass, then the batched GCW eigen-solve) and the mean
rotation error in degrees (Rotation_Alignment against the ground truth), the column of Demo/compare_algorithms.m.
Every rotation curve is scored by Rotation_Alignment_batch: the curves that share the ground truth go into one call, whose time is
printed next to the solver's.
--refined: the headline row, DESC() itself -- one DESC_batch call (the two passes of DESC_init_batch, then the batched reweighted
refinement) and the mean rotation error of R_est next to that of its initialisation R_init.
--baselines: the curves DESC is drawn against, one batched call per curve -- CEMP's SVec error (CEMP_batch) and the rotation errors of
CEMP+GCW (CEMP_GCW_batch) and CEMP+MST (CEMP_MST_batch), with the demo's CEMP parameters (compare_algorithms.m:26-29).
--mpls: the MPLS curve from one MPLS_batch call (CEMP's rounds, the tree, then the MPLS loop of every problem in one launch), with the
demo's CEMP and MPLS parameters (compare_algorithms.m:26-36): the mean rotation error of R_est next to that of its CEMP+MST start.
--lp: the linprog_sij curve from one linprog_sij_batch call (the LP of every problem in one batched PDHG loop, then the batched weighted
spectral step and refinement): mean |S_vec - ErrVec|, the mean rotation error of R_est next to that of its spectral start, and the
PDHG steps of the fastest and the slowest problem per q.
--irls: the IRLS-GM and IRLS-L0.5 curves, one IRLS_GM_batch and one IRLS_L12_batch call (a workgroup per problem runs the L1 stage and
the reweighted stage in one launch): the mean rotation error of each next to that of the L1 stage they share, and the IRLS steps.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from desc_amd import (CEMP_GCW_batch, CEMP_MST_batch, CEMP_batch, ConstantStepSize, DESC_PGD_batch, DESC_batch,  # noqa: E402
                      DESC_init_batch, IRLS_GM_batch, IRLS_L12_batch, MPLS_batch, ProblemBatch, Rotation_Alignment_batch, Uniform_Topology,
                      Uniform_Topology_batch, linprog_sij_batch)


def score(curves, models, shape):
    """The mean rotation errors (degrees) of several curves against one ground truth in ONE Rotation_Alignment_batch call: the curves'
    estimates behind one another, the models repeated.  Nodes a solver left NaN (IRLS, outside the largest component) are masked here,
    as the call requires.  Returns the curves' errors, each reshaped to (q, trial), and the call's time in ms."""
    est, gt = [], []
    for curve in curves:
        for R, mo in zip(curve, models):
            keep = np.isfinite(R).all(axis=(0, 1))
            est.append(R if keep.all() else R[:, :, keep])
            gt.append(mo if keep.all() else mo.R_orig[:, :, keep])
    t0 = time.perf_counter()
    out = Rotation_Alignment_batch(est, gt, rotations=False)
    ms = (time.perf_counter() - t0) * 1e3
    B = len(models)
    return [np.array([t[2] for t in out[k * B:(k + 1) * B]]).reshape(shape) for k in range(len(curves))], ms


def baselines(models, qs, trials, eig):
    """One call per curve: CEMP_batch, CEMP_GCW_batch, CEMP_MST_batch."""
    cemp = dict(max_iter=6, reweighting=[2.0 ** k for k in range(6)], nsample=50, seed=0)
    t0 = time.perf_counter()
    S = CEMP_batch(models, cemp)
    t1 = time.perf_counter()
    R_gcw = CEMP_GCW_batch(models, cemp, eig=eig)
    t2 = time.perf_counter()
    R_mst = CEMP_MST_batch(models, cemp)
    t3 = time.perf_counter()
    shape = (len(qs), trials)
    err = np.array([np.abs(s - mo.ErrVec).mean() for s, mo in zip(S, models)]).reshape(shape)
    (gcw, mst), ms_score = score([R_gcw, R_mst], models, shape)
    print(f"baselines, one call per curve: CEMP_batch {(t1 - t0) * 1e3:.1f} ms, CEMP_GCW_batch {(t2 - t1) * 1e3:.1f} ms, "
          f"CEMP_MST_batch {(t3 - t2) * 1e3:.1f} ms; scoring both rotation curves in one Rotation_Alignment_batch call {ms_score:.1f} ms")
    print("    q   CEMP mean |SVec - ErrVec|   CEMP+GCW rotation error, degrees   CEMP+MST rotation error, degrees   (means over the trials)")
    for q, a, b, c in zip(qs, err, gcw, mst):
        print(f" {q:4.2f}   {a.mean():.4f}                     {b.mean():8.4f}                           {c.mean():8.4f}")


def mpls_curve(models, qs, trials):
    """One MPLS_batch call: the MPLS curve of the demo."""
    cemp = dict(max_iter=6, reweighting=[2.0 ** k for k in range(6)], nsample=50, seed=0)
    mpls = dict(stop_threshold=1e-3, max_iter=100, reweighting=cemp["reweighting"][-1], thresholding=[0.95, 0.9, 0.85, 0.8],
                cycle_info_ratio=1.0 / (np.arange(1, 101) + 1))
    t0 = time.perf_counter()
    out = MPLS_batch(models, cemp, mpls, return_info=True)
    ms = (time.perf_counter() - t0) * 1e3
    shape = (len(qs), trials)
    (est, ini), ms_score = score([[R for R, _, _ in out], [R for _, R, _ in out]], models, shape)
    print(f"MPLS, {len(models)} problems in one MPLS_batch call: {ms:.1f} ms (the loop's launch {out[0][2]['mpls']['timings']['ms_loop']:.1f} ms); "
          f"scoring in one Rotation_Alignment_batch call {ms_score:.1f} ms")
    its = np.array([info["mpls"]["iters"] for _, _, info in out]).reshape(shape)
    print("    q   MPLS rotation error, degrees   (min .. max)          its initialisation's (CEMP+MST)   iterations (min .. max)")
    for q, re, ri, ni in zip(qs, est, ini, its):
        print(f" {q:4.2f}   {re.mean():8.4f}                       ({re.min():.4f} .. {re.max():.4f})      {ri.mean():8.4f}                          {ni.min()} .. {ni.max()}")


def lp_curve(models, qs, trials, eig):
    """One linprog_sij_batch call: the LP relaxation of the problem DESC solves as a QP."""
    t0 = time.perf_counter()
    out = linprog_sij_batch(models, dict(seed=0), return_info=True, eig=eig)
    ms = (time.perf_counter() - t0) * 1e3
    shape = (len(qs), trials)
    err = np.array([np.abs(s - mo.ErrVec).mean() for (_, s, _), mo in zip(out, models)]).reshape(shape)
    (est, ini), ms_score = score([[R for R, _, _ in out], [info["R_gcw"] for _, _, info in out]], models, shape)
    print(f"linprog_sij, {len(models)} problems in one linprog_sij_batch call: {ms:.1f} ms (the LP loop {out[0][2]['lp']['timings']['ms_loop']:.1f} ms); "
          f"scoring in one Rotation_Alignment_batch call {ms_score:.1f} ms")
    its = np.array([info["lp"]["iters"] for _, _, info in out]).reshape(shape)
    print("    q   mean |S_vec - ErrVec|   linprog_sij rotation error, degrees   its spectral start's (R_gcw)   PDHG steps (min .. max)")
    for q, e, re, ri, ni in zip(qs, err, est, ini, its):
        print(f" {q:4.2f}   {e.mean():.4f}                  {re.mean():8.4f}                              {ri.mean():8.4f}                       {ni.min()} .. {ni.max()}")


def irls_curves(models, qs, trials):
    """One call per curve: IRLS_GM_batch, IRLS_L12_batch (the demo's defaults: SIGMA = 5 degrees, MaxIterations = [10, 100])."""
    t0 = time.perf_counter()
    gm = IRLS_GM_batch(models, return_info=True)
    t1 = time.perf_counter()
    l12 = IRLS_L12_batch(models, return_info=True)
    t2 = time.perf_counter()
    shape = (len(qs), trials)
    (e_gm, e_l12, e_l1), ms_score = score([[R for R, _ in gm], [R for R, _ in l12], [info["R_l1"] for _, info in gm]], models, shape)
    print(f"IRLS, {len(models)} problems, one call per curve: IRLS_GM_batch {(t1 - t0) * 1e3:.1f} ms (its solve launch "
          f"{gm[0][1]['timings']['ms_solve']:.1f} ms), IRLS_L12_batch {(t2 - t1) * 1e3:.1f} ms; scoring the three curves in one "
          f"Rotation_Alignment_batch call {ms_score:.1f} ms")
    n_gm = np.array([info["irls_iters"] for _, info in gm]).reshape(shape)
    n_l12 = np.array([info["irls_iters"] for _, info in l12]).reshape(shape)
    print("    q   IRLS-GM rotation error, degrees   IRLS-L0.5 rotation error, degrees   their L1 start's (R_l1)   IRLS steps GM / L0.5 (min .. max)")
    for q, a, b, c, na, nb in zip(qs, e_gm, e_l12, e_l1, n_gm, n_l12):
        print(f" {q:4.2f}   {a.mean():8.4f}                          {b.mean():8.4f}                            {c.mean():8.4f}"
              f"                  {na.min()} .. {na.max()} / {nb.min()} .. {nb.max()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--build", choices=("host", "device"), default="host", help="where the batch's cycle structures are built")
    ap.add_argument("--rotations", action="store_true", help="one DESC_init_batch call: the mean rotation error next to the S_vec error")
    ap.add_argument("--refined", action="store_true", help="one DESC_batch call: the rotation error of DESC() next to its initialisation's")
    ap.add_argument("--baselines", action="store_true", help="CEMP, CEMP+GCW and CEMP+MST next to DESC: one batched call per curve")
    ap.add_argument("--mpls", action="store_true", help="the MPLS curve: one MPLS_batch call")
    ap.add_argument("--lp", action="store_true", help="the linprog_sij curve: one linprog_sij_batch call")
    ap.add_argument("--irls", action="store_true", help="the IRLS-GM and IRLS-L0.5 curves: one IRLS_GM_batch and one IRLS_L12_batch call")
    ap.add_argument("--device-models", action="store_true", help="draw the trials on the GPU: one Uniform_Topology_batch call")
    ap.add_argument("--resident", action="store_true", help="one ProblemBatch for every curve: the problems stay on the GPU across the calls")
    ap.add_argument("--eig", choices=("lds", "streamed", "auto"), default="lds",
                    help="the batched eigen-solve's blocks: in LDS (up to 278 nodes), streamed through LDS, or by each problem's size")
    a = ap.parse_args()
    qs = [0.0, 0.1, 0.2, 0.3, 0.4, 0.5]
    t0 = time.perf_counter()
    if a.device_models:
        models = Uniform_Topology_batch(a.n, 0.5, [q for q in qs for _ in range(a.trials)], 0.1, "uniform",
                                        seeds=[1000 * k + t for k in range(len(qs)) for t in range(a.trials)], resident=a.resident)
    else:
        models = [Uniform_Topology(a.n, 0.5, q, 0.1, "uniform", seed=1000 * k + t) for k, q in enumerate(qs) for t in range(a.trials)]
    print(f"{len(models)} problems drawn by " + ("one Uniform_Topology_batch call" if a.device_models else f"{len(models)} Uniform_Topology calls on the host")
          + f": {(time.perf_counter() - t0) * 1e3:.1f} ms")
    if a.resident:
        if not a.device_models:
            t0 = time.perf_counter()
            models = ProblemBatch(models)
            print(f"wrapped as one ProblemBatch (marshalled, laid out, uploaded once): {(time.perf_counter() - t0) * 1e3:.1f} ms")
        up, down = models.bytes()
        print(f"the resident set copied {up} bytes to the device and {down} bytes back")
    params = dict(iters=a.iters, Gradient=ConstantStepSize(0.01), seed=0, verbose=False)
    if a.refined:
        t0 = time.perf_counter()
        out = DESC_batch(models, params, build=a.build, eig=a.eig)
        ms = (time.perf_counter() - t0) * 1e3
        shape = (len(qs), a.trials)
        err = np.array([np.abs(s - mo.ErrVec).mean() for (_, _, s), mo in zip(out, models)]).reshape(shape)
        (est, ini), ms_score = score([[R for R, _, _ in out], [R for _, R, _ in out]], models, shape)
        print(f"{len(models)} problems (n = {a.n}, {a.trials} trials per q) in one DESC_batch call: {ms:.1f} ms; "
              f"scoring in one Rotation_Alignment_batch call {ms_score:.1f} ms")
        print("    q   mean |S_vec - ErrVec|   DESC rotation error, degrees   (min .. max)          its initialisation's (R_init)")
        for q, row, re, ri in zip(qs, err, est, ini):
            print(f" {q:4.2f}   {row.mean():.4f}                {re.mean():8.4f}                       ({re.min():.4f} .. {re.max():.4f})      {ri.mean():8.4f}")
        if a.baselines:
            baselines(models, qs, a.trials, a.eig)
        if a.mpls:
            mpls_curve(models, qs, a.trials)
        if a.lp:
            lp_curve(models, qs, a.trials, a.eig)
        if a.irls:
            irls_curves(models, qs, a.trials)
        return
    t0 = time.perf_counter()
    if a.rotations:
        out = DESC_init_batch(models, params, build=a.build, eig=a.eig)
        S = [s for _, s in out]
    else:
        S = DESC_PGD_batch(models, params, build=a.build)
    ms = (time.perf_counter() - t0) * 1e3
    err = np.array([np.abs(s - mo.ErrVec).mean() for s, mo in zip(S, models)]).reshape(len(qs), a.trials)
    print(f"{len(models)} problems (n = {a.n}, {a.trials} trials per q) in one {'DESC_init_batch' if a.rotations else 'DESC_PGD_batch'} call: {ms:.1f} ms")
    if a.rotations:
        (rot,), ms_score = score([[R for R, _ in out]], models, (len(qs), a.trials))
        print(f"scoring in one Rotation_Alignment_batch call: {ms_score:.1f} ms")
        print("    q   mean |S_vec - ErrVec|   (min .. max)          mean rotation error, degrees   (min .. max over the trials)")
        for q, row, rr in zip(qs, err, rot):
            print(f" {q:4.2f}   {row.mean():.4f}                ({row.min():.4f} .. {row.max():.4f})      {rr.mean():8.4f}"
                  f"                      ({rr.min():.4f} .. {rr.max():.4f})")
        if a.baselines:
            baselines(models, qs, a.trials, a.eig)
        if a.mpls:
            mpls_curve(models, qs, a.trials)
        if a.lp:
            lp_curve(models, qs, a.trials, a.eig)
        if a.irls:
            irls_curves(models, qs, a.trials)
        return
    print("    q   mean |S_vec - ErrVec|   (min .. max over the trials)")
    for q, row in zip(qs, err):
        print(f" {q:4.2f}   {row.mean():.4f}                ({row.min():.4f} .. {row.max():.4f})")
    if a.baselines:
        baselines(models, qs, a.trials, a.eig)
    if a.mpls:
        mpls_curve(models, qs, a.trials)
    if a.lp:
        lp_curve(models, qs, a.trials, a.eig)
    if a.irls:
        irls_curves(models, qs, a.trials)


if __name__ == "__main__":
    main()

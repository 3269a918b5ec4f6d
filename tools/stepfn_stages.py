#!/usr/bin/env python3
"""Per-iteration cost of the two-phase iteration (a caller-supplied params.Gradient plugin, desc_pgd_ext_*) next to the fused native
sweep of the same binary, on bench.generate's C2 / C4 problems.

Per config, `--rounds` rounds alternate three legs of `--iters` iterations each (after `--warmup` untimed ones per leg):
  native       desc_pgd_iterate_timed, ConstantStepSize(lr): device time per iteration (HIP events around the whole batch)
  device mode  desc_pgd_ext_grad / torch `-lr * grad` / desc_pgd_ext_apply on device pointers: device time of the gradient pass, the
               apply pass and the objective + stop rule (HIP events, desc_pgd_ext_laps) and the wall clock per iteration
  host mode    the same with NumPy arrays: wall clock per iteration, and the share of it that is not device time of the three
               passes (the two 8 m_cycle-byte copies over PCIe, the NumPy rule and the call overhead)
There is no reorder pass to time: both kernels index the caller's vectors through src_start / seg_perm (reported as 0).

    python tools/stepfn_stages.py [--configs C2,C4] [--rounds 4] [--iters 30] [--warmup 5] [--json-dir profiles]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch          # before the library is loaded: one ROCm runtime per process (desc_amd/_lib.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from desc_amd import _lib  # noqa: E402

LR = 0.01


def params(iters, kind):
    p = _lib.default_params()
    p.iters = iters; p.step_kind = kind; p.lr = LR
    p.patience = 1 << 30; p.stop_tol = -1e300          # the stop rule never fires: every leg runs its full length
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C4")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json-dir", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in a.configs.split(","):
        mo, nn, ii, jj, rij = bench.generate(name)
        prob = _lib.ProblemArrays(nn, ii, jj, rij)
        st = _lib.Structure.build(prob, 30, 0, _lib.BUILD_DEVICE, 0)
        solver = _lib.Solver(prob, st, 0)
        st.free()
        mc, N, W = solver.m_cycle, a.iters, a.warmup
        lay = solver.layout_stats()
        grad_t = torch.empty(mc, dtype=torch.float64, device=dev)
        grad_h = np.zeros(mc)
        nat, laps_d, wall_d, laps_h, wall_h = [], [], [], [], []
        try:
            for _ in range(a.rounds):
                solver.reset(params(N + W, _lib.STEP_CONSTANT))
                solver.iterate_timed(W)
                ms, _k = solver.iterate_timed(N)
                nat.append(ms / N)
                solver.ext_begin(params(N + W, _lib.STEP_EXTERNAL))
                for it in range(N + W):
                    t0 = time.perf_counter()
                    solver.ext_grad(grad_t.data_ptr(), _lib.MEM_DEVICE)
                    step = -LR * grad_t
                    torch.cuda.current_stream(dev).synchronize()
                    solver.ext_apply(step.data_ptr(), _lib.MEM_DEVICE)
                    if it >= W:
                        wall_d.append((time.perf_counter() - t0) * 1e3); laps_d.append(solver.ext_laps())
                solver.ext_begin(params(N + W, _lib.STEP_EXTERNAL))
                for it in range(N + W):
                    t0 = time.perf_counter()
                    solver.ext_grad(grad_h, _lib.MEM_HOST)
                    step = -LR * grad_h
                    solver.ext_apply(step, _lib.MEM_HOST)
                    if it >= W:
                        wall_h.append((time.perf_counter() - t0) * 1e3); laps_h.append(solver.ext_laps())
        finally:
            solver.destroy()
        med = lambda x: float(np.median(x))          # noqa: E731
        ld, lh = np.array(laps_d), np.array(laps_h)
        two = med(ld.sum(axis=1))
        # bytes per iteration: the fused sweep as bench.py counts it; the two passes read what it reads, write and read grad and the
        # step once more each (4 x 8 B), the permutation byte in both passes, and the objective pass streams w and the packed word again
        # (the fused path gets the objective for free inside the next sweep)
        fused = 28.0 * mc + 10.0 * lay.get("colsum_entries", 0) + 12.0 * solver.m_pos
        split = fused + (16.0 + 2.0) * mc + 12.0 * mc
        rec = dict(config=name, n=int(nn), m=int(prob.m), m_pos=int(solver.m_pos), m_cycle=int(mc), iterations_per_leg=len(wall_d), rounds=a.rounds,
                   native_ms=med(nat), native_ms_rounds=nat,
                   grad_pass_ms=med(ld[:, 0]), apply_pass_ms=med(ld[:, 1]), objective_ms=med(ld[:, 2]), reorder_ms=0.0,
                   two_phase_device_ms=two, ratio_vs_native=two / med(nat),
                   ratio_rounds=[float(np.median(ld[r * N:(r + 1) * N].sum(axis=1)) / nat[r]) for r in range(a.rounds)],
                   bytes_fused=fused, bytes_two_phase=split, ratio_bytes=split / fused,
                   device_mode_wall_ms=med(wall_d), host_mode_wall_ms=med(wall_h), host_mode_device_ms=med(lh.sum(axis=1)),
                   host_mode_copy_share=1.0 - med(lh.sum(axis=1)) / med(wall_h), pcie_bytes_per_iteration=16.0 * mc)
        print(f"{name}: n={nn} m={prob.m} m_cycle={mc}  ({len(wall_d)} iterations per leg, {a.rounds} rounds alternating)")
        print(f"  native fused iteration       {rec['native_ms']:8.3f} ms   (rounds: {', '.join('%.3f' % x for x in nat)})")
        print(f"  two-phase, device time       {two:8.3f} ms   = gradient pass {rec['grad_pass_ms']:.3f} + apply pass {rec['apply_pass_ms']:.3f} + objective "
              f"{rec['objective_ms']:.3f} + reorders 0   ratio {rec['ratio_vs_native']:.2f} (rounds: {', '.join('%.2f' % x for x in rec['ratio_rounds'])}); bytes {rec['ratio_bytes']:.2f}")
        print(f"  device mode, wall clock      {rec['device_mode_wall_ms']:8.3f} ms per iteration (torch -lr * grad included)")
        print(f"  host mode, wall clock        {rec['host_mode_wall_ms']:8.3f} ms per iteration, {100 * rec['host_mode_copy_share']:.0f} % of it copies over PCIe + the NumPy rule "
              f"({16.0 * mc / 1e6:.0f} MB per iteration)")
        if a.json_dir:
            with open(os.path.join(a.json_dir, f"r08_stepfn_{name.lower()}.json"), "w") as f:
                json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()

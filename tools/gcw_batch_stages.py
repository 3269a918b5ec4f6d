#!/usr/bin/env python3
"""What the batched eigen-solve gains: one GCW_batch / DESC_init_batch call against B consecutive GCW() / DESC_init() calls on the same arrays.

Workloads: n = 100 with B = 1, 16, 64, 256 and n = 200 with B = 16, 64; problems Uniform_Topology(n, 0.5, 0.2, 0.1), model seeds
0 .. B-1; S_vec = the PGD output after 100 iterations (lr = 0.01).  Per workload, after one warm-up of each path, the median and the
spread (min .. max) of `--reps` repetitions of the host clock:
  (a) one GCW_batch call            against  B consecutive GCW() calls,
  (b) one DESC_init_batch call      against  B consecutive DESC_init() calls,
  (c) the stage columns of the batched eigen-solve: structure / upload / eig (device time) / project / total.
Without --only the tool is a driver: every workload runs in a process of its own under its own time limit, and the first one that
fails ends the run.

    python tools/gcw_batch_stages.py [--reps 5] [--out profiles/gcw_batch_stages.json] [--only 100:64] [--timeout 240]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [(100, 1), (100, 16), (100, 64), (100, 256), (200, 16), (200, 64)]
ITERS = 100


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def measure(n, B, reps):
    from desc_amd import ConstantStepSize, DESC_PGD_batch, DESC_init, DESC_init_batch, GCW, GCW_batch, Uniform_Topology
    from oracle.spectral_oracle import rotation_alignment
    models = [Uniform_Topology(n, 0.5, 0.2, 0.1, "uniform", seed=s) for s in range(B)]
    par = lambda: dict(iters=ITERS, Gradient=ConstantStepSize(0.01), seed=0, verbose=False)      # noqa: E731
    S = DESC_PGD_batch(models, par())
    GCW_batch(models, S); DESC_init_batch(models, par())                                          # warm-up (code objects, block caches)
    GCW(models[0].Ind, None, models[0].RijMat, S[0]); DESC_init(models[0].Ind, models[0].RijMat, par())
    t = dict(gcw_batch=[], gcw_single=[], init_batch=[], init_single=[])
    stages, Rb, Rs = [], None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = GCW_batch(models, S, return_info=True)
        t["gcw_batch"].append((time.perf_counter() - t0) * 1e3)
        stages.append(out[0][1]["timings"])
        t0 = time.perf_counter()
        Rs = [GCW(mo.Ind, None, mo.RijMat, s) for mo, s in zip(models, S)]
        t["gcw_single"].append((time.perf_counter() - t0) * 1e3)
        Rb = [R for R, _ in out]
        t0 = time.perf_counter()
        DESC_init_batch(models, par())
        t["init_batch"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for mo in models:
            DESC_init(mo.Ind, mo.RijMat, par())
        t["init_single"].append((time.perf_counter() - t0) * 1e3)
    dev = max(float(np.abs(rotation_alignment(a, b)[0] - b).max()) for a, b in zip(Rb, Rs))
    return dict(n=n, B=B, iters=ITERS, converged=all(i["converged"] for _, i in out), products=[i["products"] for _, i in out][:8],
                a_gcw_batch_ms=stats(t["gcw_batch"]), a_gcw_single_calls_ms=stats(t["gcw_single"]),
                ratio_a_single_over_batch=float(np.median(t["gcw_single"]) / np.median(t["gcw_batch"])),
                b_init_batch_ms=stats(t["init_batch"]), b_init_single_calls_ms=stats(t["init_single"]),
                ratio_b_single_over_batch=float(np.median(t["init_single"]) / np.median(t["init_batch"])),
                c_stages_ms={k: stats([s[k] for s in stages]) for k in ("ms_structure", "ms_upload", "ms_eig", "ms_project", "ms_total")},
                max_aligned_diff_batch_vs_single=dev)


def show(r):
    c = r["c_stages_ms"]
    print(f"n={r['n']} B={r['B']:4d}  (a) GCW_batch {r['a_gcw_batch_ms']['median']:8.2f} ms [{r['a_gcw_batch_ms']['min']:.2f} .. {r['a_gcw_batch_ms']['max']:.2f}]  "
          f"{r['B']} x GCW {r['a_gcw_single_calls_ms']['median']:9.2f} ms  ratio {r['ratio_a_single_over_batch']:.2f}   "
          f"(b) DESC_init_batch {r['b_init_batch_ms']['median']:8.2f} ms  {r['B']} x DESC_init {r['b_init_single_calls_ms']['median']:9.2f} ms  "
          f"ratio {r['ratio_b_single_over_batch']:.2f}", flush=True)
    print(f"      (c) structure {c['ms_structure']['median']:.2f}  upload {c['ms_upload']['median']:.2f}  eig {c['ms_eig']['median']:.2f}  "
          f"project {c['ms_project']['median']:.2f}  total {c['ms_total']['median']:.2f} ms   |batch - single| {r['max_aligned_diff_batch_vs_single']:.1e}  "
          f"converged {r['converged']}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="n:B, e.g. 100:64: measure this workload in this process and print its JSON row")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per workload (driver mode)")
    a = ap.parse_args()
    if a.only:
        n, B = (int(x) for x in a.only.split(":"))
        row = measure(n, B, a.reps)
        show(row)
        print("ROW " + json.dumps(row), flush=True)
        return 0
    rows = []
    for n, B in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--only", f"{n}:{B}", "--reps", str(a.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        for line in p.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
            else:
                print(line, flush=True)
        if p.returncode != 0:
            print(f"workload {n}:{B} ended with status {p.returncode}: stopping here", flush=True)
            break
    if a.out and rows:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/gcw_batch_stages.py", reps=a.reps, rows=rows), f, indent=1)
            f.write("\n")
    return 0 if len(rows) == len(WORKLOADS) else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""What the batched IRLS gains: one IRLS_GM_batch (IRLS_L12_batch) call against B consecutive IRLS_GM() (IRLS_L12()) calls of the single
path on the same problems.

Workloads: n = 100 with B = 1, 16, 64, 256 and n = 200 with B = 16, 64; problems Uniform_Topology(n, 0.5, 0.2, 0.1), model seeds
0 .. B-1 (all connected); the demo's defaults SIGMA = 5, MaxIterations = [10, 100].  Per workload and mode, after one warm-up of each
path, the median and the spread (min .. max) of `--reps` repetitions of the host clock, the two paths in alternating order:
  (a) one batched call              against  B consecutive single calls,
  (b) the stage columns of the batched call: create's structure / upload, the projection launch with its read-back, the solve launch
      (device time), the call's total.
The row also says whether (a)'s two sides agree bit for bit (R, R_l1 and every count and score of the record), and the L1, IRLS and
PCG steps of the batch.  Without --only the tool is a driver: every workload runs in a process of its own under its own time limit,
and the first one that fails ends the run.

    python tools/irls_batch_stages.py [--reps 5] [--out profiles/irls_batch_stages.json] [--only 100:64] [--timeout 240]
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
STAGES = ("ms_structure", "ms_upload", "ms_project", "ms_solve", "ms_total")
KEYS = ("l1_iters", "irls_iters", "l1_score", "irls_score", "pd_steps", "pd_ill", "pd_stuck", "pd_solves", "cg_iters_l1", "cg_iters_irls",
        "cg_unconverged", "cg_residual", "warned_edges", "comp_nodes", "comp_edges")


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def measure_mode(mode, models, reps):
    import desc_amd
    B = len(models)
    batch_fn = getattr(desc_amd, f"IRLS_{mode}_batch")
    single_fn = getattr(desc_amd, f"IRLS_{mode}")
    batch_fn(models)                                                                              # warm-up (code objects, block caches)
    single_fn(models[0].RijMat, models[0].Ind)
    t = dict(batch=[], single=[])
    stages, out, single = [], None, None

    def run_batch():
        nonlocal out
        t0 = time.perf_counter()
        out = batch_fn(models, return_info=True)
        t["batch"].append((time.perf_counter() - t0) * 1e3)
        stages.append(dict(out[0][1]["timings"]))

    def run_single():
        nonlocal single
        t0 = time.perf_counter()
        single = [single_fn(mo.RijMat, mo.Ind, return_info=True) for mo in models]
        t["single"].append((time.perf_counter() - t0) * 1e3)

    for rep in range(reps):
        order = (run_batch, run_single) if rep % 2 == 0 else (run_single, run_batch)              # alternating order
        for fn in order:
            fn()
    bitwise = all(np.array_equal(a[0], b[0]) and np.array_equal(a[1]["R_l1"], b[1]["R_l1"]) and all(a[1][k] == b[1][k] for k in KEYS)
                  for a, b in zip(out, single))
    return dict(batch_ms=stats(t["batch"]), single_calls_ms=stats(t["single"]),
                ratio_single_over_batch=float(np.median(t["single"]) / np.median(t["batch"])),
                stages_ms={k: stats([s[k] for s in stages]) for k in STAGES}, batch_equals_single_bitwise=bool(bitwise),
                l1_steps=[i["l1_iters"] for _, i in out][:8], irls_steps=[i["irls_iters"] for _, i in out][:8],
                cg_steps_l1=[i["cg_iters_l1"] for _, i in out], cg_steps_irls=[i["cg_iters_irls"] for _, i in out],
                irls_steps_all=[i["irls_iters"] for _, i in out], cg_unconverged=int(sum(i["cg_unconverged"] for _, i in out)))


def measure(n, B, reps):
    from desc_amd import Uniform_Topology
    models = [Uniform_Topology(n, 0.5, 0.2, 0.1, "uniform", seed=s) for s in range(B)]
    return dict(n=n, B=B, reps=reps, GM=measure_mode("GM", models, reps), L12=measure_mode("L12", models, reps))


def show(r):
    for mode in ("GM", "L12"):
        d = r[mode]
        c = d["stages_ms"]
        print(f"n={r['n']} B={r['B']:4d}  (a) IRLS_{mode}_batch {d['batch_ms']['median']:8.2f} ms [{d['batch_ms']['min']:.2f} .. {d['batch_ms']['max']:.2f}]  "
              f"{r['B']} x IRLS_{mode} {d['single_calls_ms']['median']:9.2f} ms [{d['single_calls_ms']['min']:.2f} .. {d['single_calls_ms']['max']:.2f}] "
              f" ratio {d['ratio_single_over_batch']:.2f}", flush=True)
        print("      (b) " + "  ".join(f"{k[3:]} {c[k]['median']:.2f}" for k in STAGES) +
              f" ms   bitwise {d['batch_equals_single_bitwise']}  L1 steps {d['l1_steps']}  IRLS steps {d['irls_steps']}  PCG unconverged {d['cg_unconverged']}",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="n:B, e.g. 100:64: measure this workload in this process and print its JSON row")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per workload of up to 64 problems (driver mode); B / 64 times as long above")
    a = ap.parse_args()
    if a.only:
        n, B = (int(x) for x in a.only.split(":"))
        row = measure(n, B, a.reps)
        show(row)
        print("ROW " + json.dumps(row), flush=True)
        return 0 if row["GM"]["batch_equals_single_bitwise"] and row["L12"]["batch_equals_single_bitwise"] else 1
    rows = []
    for n, B in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(a.timeout * max(1, B // 64)), sys.executable, os.path.abspath(__file__), "--only", f"{n}:{B}", "--reps", str(a.reps)]
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
            json.dump(dict(tool="tools/irls_batch_stages.py", reps=a.reps, rows=rows), f, indent=1)
            f.write("\n")
    return 0 if len(rows) == len(WORKLOADS) else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""What the batched linprog_sij gains: one linprog_sij_batch call against B consecutive linprog_sij() calls on the same problems.

Workloads: n = 100 with B = 1, 16, 64 and n = 200 with B = 16; problems Uniform_Topology(n, 0.5, 0.2, 0.1), model seeds 0 .. B-1; default
parameters (tol 1e-4, max_iter 200000, check_every 64, restarts, nsample by the rule), sampling seed 0 for every problem.  Per workload,
after one warm-up of each path, `--reps` repetitions in alternating order (batch, singles, batch, ...) of the host clock; the row holds
the median and the spread (min .. max) of
  (a) one linprog_sij_batch call    against  B consecutive linprog_sij() calls (the baseline: the single path, never the batch itself),
  (b) the stage split of the batched call: the LP's create (structure / upload / build) and loop, the spectral step, the refinement,
and the PDHG steps of the fastest and the slowest problem.  The tool asserts that the two sides agree bit for bit in S_vec.  Without
--only it is a driver: every workload runs in a process of its own under its own time limit, and the first one that fails ends the run.

    python tools/lp_batch_stages.py [--reps 5] [--out profiles/lp_batch_stages.json] [--only 100:64] [--timeout 400]
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

WORKLOADS = [(100, 1), (100, 16), (100, 64), (200, 16)]
LP_STAGES = ("ms_structure", "ms_upload", "ms_build", "ms_loop")


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def measure(n, B, reps):
    from desc_amd import Uniform_Topology, linprog_sij, linprog_sij_batch
    models = [Uniform_Topology(n, 0.5, 0.2, 0.1, "uniform", seed=s) for s in range(B)]
    prm = dict(seed=0)
    linprog_sij_batch(models, prm)                                                                # warm-up (code objects, block caches)
    linprog_sij(models[0].Ind, models[0].RijMat, prm)
    t = dict(batch=[], single=[])
    stages, out, single = [], None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = linprog_sij_batch(models, prm, return_info=True)
        t["batch"].append((time.perf_counter() - t0) * 1e3)
        info = out[0][2]
        stages.append(dict({k: info["lp"]["timings"][k] for k in LP_STAGES}, ms_spectral=info["spectral"]["timings"]["ms_total"],
                           ms_refine=info["refine"]["timings"]["ms_total"]))
        t0 = time.perf_counter()
        single = [linprog_sij(mo.Ind, mo.RijMat, prm) for mo in models]
        t["single"].append((time.perf_counter() - t0) * 1e3)
    bitwise = all(np.array_equal(a[1], b[1]) for a, b in zip(out, single))
    assert bitwise, "S_vec of the batched call differs from linprog_sij's"
    steps = [i["lp"]["iters"] for _, _, i in out]
    return dict(n=n, B=B, reps=reps, nsample=[int(i["lp"]["nsample"]) for _, _, i in out][:4], lp_steps_min=int(min(steps)), lp_steps_max=int(max(steps)),
                converged=int(sum(i["lp"]["converged"] for _, _, i in out)), a_lp_batch_ms=stats(t["batch"]), a_lp_single_calls_ms=stats(t["single"]),
                ratio_a_single_over_batch=float(np.median(t["single"]) / np.median(t["batch"])),
                b_stages_ms={k: stats([s[k] for s in stages]) for k in stages[0]}, s_vec_equals_single_bitwise=bool(bitwise))


def show(r):
    c = r["b_stages_ms"]
    print(f"n={r['n']} B={r['B']:3d}  (a) linprog_sij_batch {r['a_lp_batch_ms']['median']:9.2f} ms [{r['a_lp_batch_ms']['min']:.2f} .. {r['a_lp_batch_ms']['max']:.2f}]  "
          f"{r['B']} x linprog_sij {r['a_lp_single_calls_ms']['median']:9.2f} ms [{r['a_lp_single_calls_ms']['min']:.2f} .. {r['a_lp_single_calls_ms']['max']:.2f}]  "
          f"ratio {r['ratio_a_single_over_batch']:.2f}", flush=True)
    print("      (b) create " + "  ".join(f"{k[3:]} {c[k]['median']:.2f}" for k in LP_STAGES[:3]) + f"   LP loop {c['ms_loop']['median']:.2f}   spectral "
          f"{c['ms_spectral']['median']:.2f}   refinement {c['ms_refine']['median']:.2f} ms   steps {r['lp_steps_min']} .. {r['lp_steps_max']}  "
          f"converged {r['converged']}/{r['B']}  S_vec bitwise {r['s_vec_equals_single_bitwise']}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="n:B, e.g. 100:64: measure this workload in this process and print its JSON row")
    ap.add_argument("--timeout", type=int, default=400, help="seconds per workload (driver mode)")
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
            json.dump(dict(tool="tools/lp_batch_stages.py", reps=a.reps, rows=rows), f, indent=1)
            f.write("\n")
    return 0 if len(rows) == len(WORKLOADS) else 1


if __name__ == "__main__":
    sys.exit(main())

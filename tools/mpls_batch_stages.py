#!/usr/bin/env python3
"""What the batched MPLS gains: one MPLS_batch call against B consecutive MPLS() calls of the single path on the same problems.

Workloads: n = 100 with B = 1, 16, 64, 256 and n = 200 with B = 16, 64; problems Uniform_Topology(n, 0.5, 0.2, 0.1), model seeds
0 .. B-1; the parameters of Demo/compare_algorithms.m:26-36 with nsample = 50, sampling seed 0 for every problem.  Per workload, after
one warm-up of each path, the median and the spread (min .. max) of `--reps` repetitions of the host clock (the B single calls, which
take seconds for a large batch, are repeated reps * 64 / B times, at least twice, once B exceeds 64; the row says how often):
  (a) one MPLS_batch call           against  B consecutive MPLS() calls,
  (b) the stage columns of the batched call: CEMP's create (structure / upload / build) and rounds, the tree pass, and the loop's
      setup / input / loop (device time) / download / total.
The row also says whether (a)'s two sides agree bit for bit (R_est, R_init, iters, score, cg_iters), and the MPLS and PCG steps of the
batch.  Without --only the tool is a driver: every workload runs in a process of its own under its own time limit, and the first one
that fails ends the run.

    python tools/mpls_batch_stages.py [--reps 5] [--out profiles/mpls_batch_stages.json] [--only 100:64] [--timeout 240]
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
NSAMPLE = 50
CEMP_STAGES = ("ms_structure", "ms_upload", "ms_build", "ms_rounds")
MPLS_STAGES = ("ms_setup", "ms_input", "ms_loop", "ms_download", "ms_total")


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def demo_params():
    """Demo/compare_algorithms.m:26-36."""
    cemp = dict(max_iter=6, reweighting=[2.0 ** k for k in range(6)], nsample=NSAMPLE, seed=0)
    mpls = dict(stop_threshold=1e-3, max_iter=100, reweighting=cemp["reweighting"][-1], thresholding=[0.95, 0.9, 0.85, 0.8],
                cycle_info_ratio=1.0 / (np.arange(1, 101) + 1))
    return cemp, mpls


def measure(n, B, reps):
    from desc_amd import MPLS, MPLS_batch, Uniform_Topology
    models = [Uniform_Topology(n, 0.5, 0.2, 0.1, "uniform", seed=s) for s in range(B)]
    cemp, mpls = demo_params()
    MPLS_batch(models, cemp, mpls)                                                                # warm-up (code objects, block caches)
    MPLS(models[0].Ind, models[0].RijMat, cemp, mpls)
    t = dict(batch=[], single=[])
    stages, out, single = [], None, None
    single_reps = reps if B <= 64 else max(2, reps * 64 // B)
    for rep in range(reps):
        t0 = time.perf_counter()
        out = MPLS_batch(models, cemp, mpls, return_info=True)
        t["batch"].append((time.perf_counter() - t0) * 1e3)
        info = out[0][2]
        stages.append(dict({k: info["cemp"]["timings"][k] for k in CEMP_STAGES}, ms_mst=info["mst"]["timings"]["ms_total"],
                           **{k: info["mpls"]["timings"][k] for k in MPLS_STAGES}))
        if rep < single_reps:
            t0 = time.perf_counter()
            single = [MPLS(mo.Ind, mo.RijMat, cemp, mpls, return_info=True) for mo in models]
            t["single"].append((time.perf_counter() - t0) * 1e3)
    bitwise = all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and
                  all(a[2]["mpls"][k] == b[2][k] for k in ("iters", "score", "cg_iters")) for a, b in zip(out, single))
    return dict(n=n, B=B, nsample=NSAMPLE, reps=reps, single_reps=single_reps, mpls_steps=[i["mpls"]["iters"] for _, _, i in out][:8],
                cg_steps=[i["mpls"]["cg_iters"] for _, _, i in out][:8], cg_unconverged=int(sum(i["mpls"]["cg_unconverged"] for _, _, i in out)),
                a_mpls_batch_ms=stats(t["batch"]), a_mpls_single_calls_ms=stats(t["single"]),
                ratio_a_single_over_batch=float(np.median(t["single"]) / np.median(t["batch"])),
                b_stages_ms={k: stats([s[k] for s in stages]) for k in stages[0]}, batch_equals_single_bitwise=bool(bitwise))


def show(r):
    c = r["b_stages_ms"]
    print(f"n={r['n']} B={r['B']:4d}  (a) MPLS_batch {r['a_mpls_batch_ms']['median']:8.2f} ms [{r['a_mpls_batch_ms']['min']:.2f} .. {r['a_mpls_batch_ms']['max']:.2f}]  "
          f"{r['B']} x MPLS {r['a_mpls_single_calls_ms']['median']:9.2f} ms [{r['a_mpls_single_calls_ms']['min']:.2f} .. {r['a_mpls_single_calls_ms']['max']:.2f}] "
          f"({r['single_reps']} reps)  ratio {r['ratio_a_single_over_batch']:.2f}", flush=True)
    print("      (b) CEMP " + "  ".join(f"{k[3:]} {c[k]['median']:.2f}" for k in CEMP_STAGES) + f"   tree {c['ms_mst']['median']:.2f}   loop " +
          "  ".join(f"{k[3:]} {c[k]['median']:.2f}" for k in MPLS_STAGES) +
          f" ms   bitwise {r['batch_equals_single_bitwise']}  steps {r['mpls_steps']}  PCG unconverged {r['cg_unconverged']}", flush=True)


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
        return 0
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
            json.dump(dict(tool="tools/mpls_batch_stages.py", reps=a.reps, rows=rows), f, indent=1)
            f.write("\n")
    return 0 if len(rows) == len(WORKLOADS) else 1


if __name__ == "__main__":
    sys.exit(main())

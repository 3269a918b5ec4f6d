#!/usr/bin/env python3
"""What the batched CEMP baselines gain: one CEMP_batch / CEMP_GCW_batch / CEMP_MST_batch call against B consecutive CEMP() / CEMP_GCW()
/ MST(CEMP()) calls on the same arrays.

Workloads: n = 100 with B = 1, 16, 64, 256 and n = 200 with B = 16, 64; problems Uniform_Topology(n, 0.5, 0.2, 0.1), model seeds
0 .. B-1; the demo's CEMP parameters (max_iter = 6, reweighting = 2 ** (0..5), nsample = 50).  Per workload, after one warm-up of each
path, the median and the spread (min .. max) of `--reps` repetitions of the host clock:
  (a) one CEMP_batch call           against  B consecutive CEMP() calls,
  (b) one CEMP_GCW_batch call       against  B consecutive CEMP_GCW() calls,
  (c) one CEMP_MST_batch call       against  B consecutive MST(CEMP()) calls (the initialisation of MPLS),
  (d) the stage columns of the batched CEMP (structure / upload / build / rounds / total) and of the batched tree step
      (structure / upload / tree / propagate / total).
Without --only the tool is a driver: every workload runs in a process of its own under its own time limit, and the first one that
fails ends the run.

    python tools/cemp_batch_stages.py [--reps 5] [--out profiles/cemp_batch_stages.json] [--only 100:64] [--timeout 240]
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
CEMP_STAGES = ("ms_structure", "ms_upload", "ms_build", "ms_rounds", "ms_total")
MST_STAGES = ("ms_structure", "ms_upload", "ms_tree", "ms_propagate", "ms_total")


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def measure(n, B, reps):
    from desc_amd import CEMP, CEMP_GCW, CEMP_GCW_batch, CEMP_MST_batch, CEMP_batch, MST, Uniform_Topology
    models = [Uniform_Topology(n, 0.5, 0.2, 0.1, "uniform", seed=s) for s in range(B)]
    par = dict(max_iter=6, reweighting=[2.0 ** k for k in range(6)], nsample=50, seed=0)
    singles = dict(cemp=lambda: [CEMP(mo.Ind, mo.RijMat, par) for mo in models],
                   gcw=lambda: [CEMP_GCW(mo.Ind, mo.RijMat, par) for mo in models],
                   mst=lambda: [MST(mo.Ind, mo.RijMat, CEMP(mo.Ind, mo.RijMat, par)) for mo in models])
    batches = dict(cemp=lambda: CEMP_batch(models, par, return_info=True), gcw=lambda: CEMP_GCW_batch(models, par, return_info=True),
                   mst=lambda: CEMP_MST_batch(models, par, return_info=True))
    for k in batches:                                                       # warm-up (code objects, block caches)
        batches[k]()
    mo = models[0]
    CEMP_GCW(mo.Ind, mo.RijMat, par); MST(mo.Ind, mo.RijMat, CEMP(mo.Ind, mo.RijMat, par))
    t = {f"{k}_{w}": [] for k in singles for w in ("batch", "single")}
    cemp_stages, mst_stages, last = [], [], {}
    for _ in range(reps):
        for k in singles:
            ob, ms = clock(batches[k]); t[k + "_batch"].append(ms)
            os_, ms = clock(singles[k]); t[k + "_single"].append(ms)
            last[k] = (ob, os_)
        cemp_stages.append(last["cemp"][0][0][1]["timings"])
        mst_stages.append(last["mst"][0][0][2]["mst"]["timings"])
    equal = dict(cemp=all(np.array_equal(a[0], b) for a, b in zip(*last["cemp"])), mst=all(np.array_equal(a[0], b) for a, b in zip(*last["mst"])))
    row = dict(n=n, B=B, nsample=50, max_iter=6, bit_equal_to_single=equal)
    for k, name in (("cemp", "a_cemp"), ("gcw", "b_cemp_gcw"), ("mst", "c_cemp_mst")):
        row[name + "_batch_ms"] = stats(t[k + "_batch"]); row[name + "_single_calls_ms"] = stats(t[k + "_single"])
        row["ratio_" + name + "_single_over_batch"] = float(np.median(t[k + "_single"]) / np.median(t[k + "_batch"]))
    row["d_cemp_stages_ms"] = {k: stats([s[k] for s in cemp_stages]) for k in CEMP_STAGES}
    row["d_mst_stages_ms"] = {k: stats([s[k] for s in mst_stages]) for k in MST_STAGES}
    return row


def show(r):
    for name, label, single in (("a_cemp", "CEMP_batch", "CEMP"), ("b_cemp_gcw", "CEMP_GCW_batch", "CEMP_GCW"), ("c_cemp_mst", "CEMP_MST_batch", "MST(CEMP)")):
        b, s = r[name + "_batch_ms"], r[name + "_single_calls_ms"]
        print(f"n={r['n']} B={r['B']:4d}  {label:15s} {b['median']:8.2f} ms [{b['min']:.2f} .. {b['max']:.2f}]   {r['B']} x {single:9s} {s['median']:9.2f} ms "
              f"[{s['min']:.2f} .. {s['max']:.2f}]   ratio {r['ratio_' + name + '_single_over_batch']:.2f}", flush=True)
    c, m = r["d_cemp_stages_ms"], r["d_mst_stages_ms"]
    print("      CEMP stages: " + "  ".join(f"{k[3:]} {c[k]['median']:.2f}" for k in CEMP_STAGES) + " ms;  tree stages: "
          + "  ".join(f"{k[3:]} {m[k]['median']:.2f}" for k in MST_STAGES) + f" ms;  bit-equal to the single calls: {r['bit_equal_to_single']}", flush=True)


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
            json.dump(dict(tool="tools/cemp_batch_stages.py", reps=a.reps, rows=rows), f, indent=1)
            f.write("\n")
    return 0 if len(rows) == len(WORKLOADS) else 1


if __name__ == "__main__":
    sys.exit(main())

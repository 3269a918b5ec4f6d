#!/usr/bin/env python3
"""What the batched generator gains: one Uniform_Topology_batch call against B consecutive Uniform_Topology() calls on the host.

Workloads: n = 100 with B = 1, 16, 64, 256 and n = 200 with B = 16, 64; problems (n, 0.5, 0.2, 0.1), 'uniform', seeds 0 .. B-1.  The two
sides draw the same distributions from different streams, so nothing is compared but the clock (and the edge totals are printed).
Per workload, after one warm-up of each path, `--reps` repetitions in alternating order (batch, host loop, batch, ...) of the host
clock; the row holds the median and the spread (min .. max) of
  (a) one Uniform_Topology_batch call    against  B consecutive Uniform_Topology() calls (the baseline: the NumPy generator timed in
      the same process, never the batched call against itself),
  (b) the stage split of the batched call from its timings: graph pass (create), node pass, edge pass, copy-back.
Without --only it is a driver: every workload runs in a process of its own under its own time limit, and the first one that fails ends
the run.

    python tools/models_batch_stages.py [--reps 5] [--out profiles/models_batch_stages.json] [--only 100:64] [--timeout 300]
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
STAGES = ("ms_graph", "ms_nodes", "ms_edges", "ms_copy", "ms_total")


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def measure(n, B, reps):
    from desc_amd import Uniform_Topology, Uniform_Topology_batch
    seeds = list(range(B))
    Uniform_Topology_batch(n, 0.5, 0.2, 0.1, "uniform", seeds=seeds)                              # warm-up (code objects, block caches)
    Uniform_Topology(n, 0.5, 0.2, 0.1, "uniform", seed=0)
    t = dict(batch=[], host=[])
    stages, m_batch, m_host = [], 0, 0
    for _ in range(reps):
        t0 = time.perf_counter()
        mos, tm = Uniform_Topology_batch(n, 0.5, 0.2, 0.1, "uniform", seeds=seeds, return_info=True)
        t["batch"].append((time.perf_counter() - t0) * 1e3)
        stages.append(tm)
        m_batch = sum(mo.Ind.shape[0] for mo in mos)
        t0 = time.perf_counter()
        host = [Uniform_Topology(n, 0.5, 0.2, 0.1, "uniform", seed=s) for s in seeds]
        t["host"].append((time.perf_counter() - t0) * 1e3)
        m_host = sum(mo.Ind.shape[0] for mo in host)
    return dict(n=n, B=B, reps=reps, edges_batch=int(m_batch), edges_host=int(m_host), copy_bytes=int(152 * m_batch + 72 * n * B),
                a_batch_ms=stats(t["batch"]), a_host_loop_ms=stats(t["host"]), ratio_a_host_over_batch=float(np.median(t["host"]) / np.median(t["batch"])),
                b_stages_ms={k: stats([s[k] for s in stages]) for k in STAGES})


def show(r):
    c = r["b_stages_ms"]
    print(f"n={r['n']} B={r['B']:3d}  (a) Uniform_Topology_batch {r['a_batch_ms']['median']:9.2f} ms [{r['a_batch_ms']['min']:.2f} .. {r['a_batch_ms']['max']:.2f}]  "
          f"{r['B']} x Uniform_Topology {r['a_host_loop_ms']['median']:9.2f} ms [{r['a_host_loop_ms']['min']:.2f} .. {r['a_host_loop_ms']['max']:.2f}]  "
          f"ratio {r['ratio_a_host_over_batch']:.2f}", flush=True)
    print("      (b) " + "  ".join(f"{k[3:]} {c[k]['median']:.2f}" for k in STAGES) + f" ms   edges {r['edges_batch']} (host streams: {r['edges_host']})  "
          f"copy-back {r['copy_bytes'] / 1e6:.1f} MB", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="n:B, e.g. 100:64: measure this workload in this process and print its JSON row")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per workload (driver mode)")
    a = ap.parse_args()
    if a.only:
        n, B = (int(x) for x in a.only.split(":"))
        row = measure(n, B, a.reps)
        show(row)
        print("ROW " + json.dumps(row), flush=True)
        return 0
    rows, lines = [], []
    for n, B in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--only", f"{n}:{B}", "--reps", str(a.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        for line in p.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
            else:
                lines.append(line)
                print(line, flush=True)
        if p.returncode != 0:
            print(f"workload {n}:{B} ended with status {p.returncode}: stopping here", flush=True)
            break
    if a.out and rows:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/models_batch_stages.py", reps=a.reps, rows=rows), f, indent=1)
            f.write("\n")
        with open(os.path.splitext(a.out)[0] + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if len(rows) == len(WORKLOADS) else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""What the batched scoring gains: one Rotation_Alignment_batch call against B consecutive Rotation_Alignment() calls on the host.

Workloads: n = 100 with B = 1, 16, 64, 256 and n = 200 with B = 16, 64; per problem Haar ground-truth rotations and the estimates
R_gt_k * (3 degrees about a random axis) * g, seeds 0 .. B-1.  Both sides score the same arrays; the largest difference of the mean
errors is printed.  Per workload, after one warm-up of each path, `--reps` repetitions in alternating order (batch with R_out, batch
without, host loop, batch with R_out, ...) of the host clock; the row holds the median and the spread (min .. max) of
  (a) one Rotation_Alignment_batch call, rotations=True and rotations=False,  against  B consecutive Rotation_Alignment() calls (the
      baseline: the NumPy function timed in the same process, never the batched call against itself),
  (b) the stage split of the batched call from its timings: finite check and upload, the launch, copy-back.
Without --only it is a driver: every workload runs in a process of its own under its own time limit, and the first one that fails ends
the run.

    python tools/align_batch_stages.py [--reps 5] [--out profiles/align_batch_stages.json] [--only 100:64] [--timeout 300]
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
STAGES = ("ms_upload", "ms_align", "ms_copy", "ms_total")


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def haar(rng, count):
    Q, R = np.linalg.qr(rng.standard_normal((count, 3, 3)))
    Q = Q * np.sign(np.diagonal(R, axis1=1, axis2=2))[:, None, :]
    Q[:, :, 2] *= np.linalg.det(Q)[:, None]
    return Q


def problem(n, seed):
    rng = np.random.default_rng(seed)
    G, g = haar(rng, n), haar(rng, 1)[0]
    ax = rng.standard_normal((n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    t = np.deg2rad(3.0)
    E = G @ (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)) @ g
    return np.asfortranarray(np.transpose(E, (1, 2, 0))), np.asfortranarray(np.transpose(G, (1, 2, 0)))


def measure(n, B, reps):
    from desc_amd import Rotation_Alignment, Rotation_Alignment_batch
    probs = [problem(n, s) for s in range(B)]
    est, gt = [E for E, _ in probs], [G for _, G in probs]
    Rotation_Alignment_batch(est, gt)                                                            # warm-up (code objects, block caches)
    Rotation_Alignment(est[0], gt[0])
    t = dict(batch=[], bare=[], host=[])
    stages, stages_bare, diff = [], [], 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        out = Rotation_Alignment_batch(est, gt, return_info=True)
        t["batch"].append((time.perf_counter() - t0) * 1e3)
        stages.append(out[0][4]["timings"])
        t0 = time.perf_counter()
        bare = Rotation_Alignment_batch(est, gt, rotations=False, return_info=True)
        t["bare"].append((time.perf_counter() - t0) * 1e3)
        stages_bare.append(bare[0][4]["timings"])
        t0 = time.perf_counter()
        host = [Rotation_Alignment(E, G) for E, G in zip(est, gt)]
        t["host"].append((time.perf_counter() - t0) * 1e3)
        diff = max(abs(a[2] - b[2]) for a, b in zip(out, host))
    med = {k: float(np.median(v)) for k, v in t.items()}
    return dict(n=n, B=B, reps=reps, max_mean_error_difference_degrees=float(diff), copy_bytes=int(8 * B * (10 * n + 11)), copy_bytes_bare=int(8 * B * (n + 11)),
                a_batch_ms=stats(t["batch"]), a_batch_no_rotations_ms=stats(t["bare"]), a_host_loop_ms=stats(t["host"]),
                ratio_a_host_over_batch=med["host"] / med["batch"], ratio_a_host_over_batch_no_rotations=med["host"] / med["bare"],
                b_stages_ms={k: stats([s[k] for s in stages]) for k in STAGES},
                b_stages_no_rotations_ms={k: stats([s[k] for s in stages_bare]) for k in STAGES})


def show(r):
    a, b, h = r["a_batch_ms"], r["a_batch_no_rotations_ms"], r["a_host_loop_ms"]
    print(f"n={r['n']} B={r['B']:3d}  (a) Rotation_Alignment_batch {a['median']:8.3f} ms [{a['min']:.3f} .. {a['max']:.3f}]  rotations=False "
          f"{b['median']:8.3f} ms [{b['min']:.3f} .. {b['max']:.3f}]  {r['B']} x Rotation_Alignment {h['median']:8.3f} ms [{h['min']:.3f} .. {h['max']:.3f}]  "
          f"ratio {r['ratio_a_host_over_batch']:.2f} / {r['ratio_a_host_over_batch_no_rotations']:.2f}", flush=True)
    for name, c, nbytes in (("(b) with R_out   ", r["b_stages_ms"], r["copy_bytes"]), ("    rotations=False", r["b_stages_no_rotations_ms"], r["copy_bytes_bare"])):
        print(f"      {name} " + "  ".join(f"{k[3:]} {c[k]['median']:.3f}" for k in STAGES) + f" ms   copy-back {nbytes / 1e3:.1f} kB", flush=True)
    print(f"      max |mean_error - Rotation_Alignment's| = {r['max_mean_error_difference_degrees']:.2e} degrees", flush=True)


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
            json.dump(dict(tool="tools/align_batch_stages.py", reps=a.reps, rows=rows), f, indent=1)
            f.write("\n")
        with open(os.path.splitext(a.out)[0] + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if len(rows) == len(WORKLOADS) else 1


if __name__ == "__main__":
    sys.exit(main())

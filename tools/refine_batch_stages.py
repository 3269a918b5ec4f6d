#!/usr/bin/env python3
"""What the batched refinement gains: one DESC_batch / DESC_refine_batch call against B consecutive DESC() / refinement calls of the
single path on the same arrays.

Workloads: n = 100 with B = 1, 16, 64, 256 and n = 200 with B = 16, 64; problems Uniform_Topology(n, 0.5, 0.2, 0.1), model seeds
0 .. B-1; S_vec and R_init = DESC_init_batch's output after 100 PGD iterations (lr = 0.01).  Per workload, after one warm-up of each
path, the median and the spread (min .. max) of `--reps` repetitions of the host clock (the B single calls, which take seconds
for a large batch, are repeated reps * 64 / B times, at least twice, once B exceeds 64; the row says how often):
  (a) one DESC_batch call           against  B consecutive DESC() calls,
  (b) one DESC_refine_batch call    against  B consecutive _lib.refine_run calls on the same S_vec and R_init,
  (c) the stage columns of the batched refinement: structure / upload / input / refine (device time) / total.
The row also says whether (b)'s two sides agree bit for bit, and the refinement steps and PCG steps of the batch.
Without --only the tool is a driver: every workload runs in a process of its own under its own time limit, and the first one that
fails ends the run.

    python tools/refine_batch_stages.py [--reps 5] [--out profiles/refine_batch_stages.json] [--only 100:64] [--timeout 240]
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
STAGES = ("ms_structure", "ms_upload", "ms_input", "ms_refine", "ms_total")


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def measure(n, B, reps):
    from desc_amd import ConstantStepSize, DESC, DESC_batch, DESC_init_batch, DESC_refine_batch, Uniform_Topology, _lib
    from desc_amd.algorithms import marshal_edges
    models = [Uniform_Topology(n, 0.5, 0.2, 0.1, "uniform", seed=s) for s in range(B)]
    par = lambda: dict(iters=ITERS, Gradient=ConstantStepSize(0.01), seed=0, verbose=False)      # noqa: E731
    init = DESC_init_batch(models, par())
    S, R0 = [s for _, s in init], [r for r, _ in init]
    probs = []
    for mo in models:
        nn, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
        assert perm is None
        probs.append(_lib.ProblemArrays(nn, ii, jj, rij))
    DESC_refine_batch(models, S, R0); DESC_batch(models, par())                                   # warm-up (code objects, block caches)
    _lib.refine_run(probs[0], S[0], R0[0]); DESC(models[0].Ind, models[0].RijMat, par())
    t = dict(refine_batch=[], refine_single=[], desc_batch=[], desc_single=[])
    stages, out, single = [], None, None
    single_reps = reps if B <= 64 else max(2, reps * 64 // B)
    for rep in range(reps):
        t0 = time.perf_counter()
        out = DESC_refine_batch(models, S, R0, return_info=True)
        t["refine_batch"].append((time.perf_counter() - t0) * 1e3)
        stages.append(out[0][1]["timings"])
        if rep < single_reps:
            t0 = time.perf_counter()
            single = [_lib.refine_run(q, s, r) for q, s, r in zip(probs, S, R0)]
            t["refine_single"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        DESC_batch(models, par())
        t["desc_batch"].append((time.perf_counter() - t0) * 1e3)
        if rep < single_reps:
            t0 = time.perf_counter()
            for mo in models:
                DESC(mo.Ind, mo.RijMat, par())
            t["desc_single"].append((time.perf_counter() - t0) * 1e3)
    bitwise = all(np.array_equal(a[0], b[0]) and a[1]["iters"] == b[1]["iters"] and a[1]["score"] == b[1]["score"] and
                  a[1]["cg_iters"] == b[1]["cg_iters"] for a, b in zip(out, single))
    return dict(n=n, B=B, iters=ITERS, reps=reps, single_reps=single_reps, refine_steps=[i["iters"] for _, i in out][:8], cg_steps=[i["cg_iters"] for _, i in out][:8],
                cg_unconverged=int(sum(i["cg_unconverged"] for _, i in out)),
                a_desc_batch_ms=stats(t["desc_batch"]), a_desc_single_calls_ms=stats(t["desc_single"]),
                ratio_a_single_over_batch=float(np.median(t["desc_single"]) / np.median(t["desc_batch"])),
                b_refine_batch_ms=stats(t["refine_batch"]), b_refine_single_calls_ms=stats(t["refine_single"]),
                ratio_b_single_over_batch=float(np.median(t["refine_single"]) / np.median(t["refine_batch"])),
                c_stages_ms={k: stats([s[k] for s in stages]) for k in STAGES}, batch_equals_single_bitwise=bool(bitwise))


def show(r):
    c = r["c_stages_ms"]
    print(f"n={r['n']} B={r['B']:4d}  (a) DESC_batch {r['a_desc_batch_ms']['median']:8.2f} ms [{r['a_desc_batch_ms']['min']:.2f} .. {r['a_desc_batch_ms']['max']:.2f}]  "
          f"{r['B']} x DESC {r['a_desc_single_calls_ms']['median']:9.2f} ms  ratio {r['ratio_a_single_over_batch']:.2f}   "
          f"(b) DESC_refine_batch {r['b_refine_batch_ms']['median']:8.2f} ms [{r['b_refine_batch_ms']['min']:.2f} .. {r['b_refine_batch_ms']['max']:.2f}]  "
          f"{r['B']} x refine_run {r['b_refine_single_calls_ms']['median']:9.2f} ms  ratio {r['ratio_b_single_over_batch']:.2f}", flush=True)
    print(f"      (c) structure {c['ms_structure']['median']:.2f}  upload {c['ms_upload']['median']:.2f}  input {c['ms_input']['median']:.2f}  "
          f"refine {c['ms_refine']['median']:.2f}  total {c['ms_total']['median']:.2f} ms   bitwise {r['batch_equals_single_bitwise']}  "
          f"steps {r['refine_steps']}  PCG unconverged {r['cg_unconverged']}", flush=True)


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
            json.dump(dict(tool="tools/refine_batch_stages.py", reps=a.reps, rows=rows), f, indent=1)
            f.write("\n")
    return 0 if len(rows) == len(WORKLOADS) else 1


if __name__ == "__main__":
    sys.exit(main())

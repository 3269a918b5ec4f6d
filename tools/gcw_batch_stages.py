#!/usr/bin/env python3
"""What the batched eigen-solve gains: one GCW_batch / DESC_init_batch call against B consecutive GCW() / DESC_init() calls on the same arrays.

Workloads: n = 100 with B = 1, 16, 64, 256, n = 200 with B = 16, 64 and, above the LDS kernel's cap, n = 400 with B = 16, 64 and
n = 748 with B = 16; problems Uniform_Topology(n, 0.5, 0.2, 0.1), model seeds 0 .. B-1; S_vec = the PGD output after 100 iterations
(lr = 0.01).  Per workload, after one warm-up of each path, the median and the spread (min .. max) of `--reps` repetitions of the
host clock, the paths taking turns inside every repetition:
  (a) one GCW_batch call            against  B consecutive GCW() calls,
  (b) one DESC_init_batch call      against  B consecutive DESC_init() calls,
  (c) the stage columns of the batched eigen-solve: structure / upload / eig (device time) / project / total,
  (d) where both kernels take the problem (n <= 278): one GCW_batch(eig="streamed") call against one GCW_batch(eig="lds") call --
      what streaming the blocks through LDS costs, and why "auto" keeps the small problems in LDS.
--eig is the mode of (a) to (c): "auto" (the default) is the LDS kernel up to 278 nodes and the streamed kernel above; "lds" skips
the workloads above 278 nodes.
Without --only the tool is a driver: every workload runs in a process of its own under its own time limit, and the first one that
fails ends the run.

    python tools/gcw_batch_stages.py [--reps 5] [--eig auto] [--out profiles/gcw_batch_stages.json] [--workloads 400:16,748:16]
                                     [--only 100:64] [--timeout 240]
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

WORKLOADS = [(100, 1), (100, 16), (100, 64), (100, 256), (200, 16), (200, 64), (400, 16), (400, 64), (748, 16)]
ITERS = 100


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def measure(n, B, reps, eig):
    from desc_amd import ConstantStepSize, DESC_PGD_batch, DESC_init, DESC_init_batch, GCW, GCW_batch, Uniform_Topology, _lib
    from oracle.spectral_oracle import rotation_alignment
    models = [Uniform_Topology(n, 0.5, 0.2, 0.1, "uniform", seed=s) for s in range(B)]
    par = lambda: dict(iters=ITERS, Gradient=ConstantStepSize(0.01), seed=0, verbose=False)      # noqa: E731
    both = n <= _lib.gcw_batch_max_n()
    S = DESC_PGD_batch(models, par())
    GCW_batch(models, S, eig=eig); DESC_init_batch(models, par(), eig=eig)                        # warm-up (code objects, block caches)
    GCW(models[0].Ind, None, models[0].RijMat, S[0]); DESC_init(models[0].Ind, models[0].RijMat, par())
    if both:
        GCW_batch(models, S, eig="streamed"); GCW_batch(models, S, eig="lds")
    t = dict(gcw_batch=[], gcw_single=[], init_batch=[], init_single=[], streamed=[], lds=[], eig_streamed=[], eig_lds=[])
    stages, Rb, Rs = [], None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = GCW_batch(models, S, return_info=True, eig=eig)
        t["gcw_batch"].append((time.perf_counter() - t0) * 1e3)
        stages.append(out[0][1]["timings"])
        t0 = time.perf_counter()
        Rs = [GCW(mo.Ind, None, mo.RijMat, s) for mo, s in zip(models, S)]
        t["gcw_single"].append((time.perf_counter() - t0) * 1e3)
        Rb = [R for R, _ in out]
        t0 = time.perf_counter()
        DESC_init_batch(models, par(), eig=eig)
        t["init_batch"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for mo in models:
            DESC_init(mo.Ind, mo.RijMat, par())
        t["init_single"].append((time.perf_counter() - t0) * 1e3)
        if both:
            for mode in ("streamed", "lds"):
                t0 = time.perf_counter()
                o = GCW_batch(models, S, return_info=True, eig=mode)
                t[mode].append((time.perf_counter() - t0) * 1e3)
                t["eig_" + mode].append(o[0][1]["timings"]["ms_eig"])
                assert all(np.array_equal(R, Rx) for (R, _), Rx in zip(o, Rb))                    # the same bits from either kernel
    dev = max(float(np.abs(rotation_alignment(a, b)[0] - b).max()) for a, b in zip(Rb, Rs))
    row = dict(n=n, B=B, iters=ITERS, eig=eig, kernel=out[0][1]["eig"], converged=all(i["converged"] for _, i in out),
               products=[i["products"] for _, i in out][:8],
               a_gcw_batch_ms=stats(t["gcw_batch"]), a_gcw_single_calls_ms=stats(t["gcw_single"]),
               ratio_a_single_over_batch=float(np.median(t["gcw_single"]) / np.median(t["gcw_batch"])),
               b_init_batch_ms=stats(t["init_batch"]), b_init_single_calls_ms=stats(t["init_single"]),
               ratio_b_single_over_batch=float(np.median(t["init_single"]) / np.median(t["init_batch"])),
               c_stages_ms={k: stats([s[k] for s in stages]) for k in ("ms_structure", "ms_upload", "ms_eig", "ms_project", "ms_total")},
               max_aligned_diff_batch_vs_single=dev)
    if both:
        row.update(d_streamed_call_ms=stats(t["streamed"]), d_lds_call_ms=stats(t["lds"]), d_streamed_eig_ms=stats(t["eig_streamed"]),
                   d_lds_eig_ms=stats(t["eig_lds"]), ratio_d_streamed_over_lds_call=float(np.median(t["streamed"]) / np.median(t["lds"])),
                   ratio_d_streamed_over_lds_eig=float(np.median(t["eig_streamed"]) / np.median(t["eig_lds"])))
    return row


def show(r):
    c = r["c_stages_ms"]
    print(f"n={r['n']} B={r['B']:4d} eig={r['eig']} ({r['kernel']})  (a) GCW_batch {r['a_gcw_batch_ms']['median']:8.2f} ms "
          f"[{r['a_gcw_batch_ms']['min']:.2f} .. {r['a_gcw_batch_ms']['max']:.2f}]  "
          f"{r['B']} x GCW {r['a_gcw_single_calls_ms']['median']:9.2f} ms  ratio {r['ratio_a_single_over_batch']:.2f}   "
          f"(b) DESC_init_batch {r['b_init_batch_ms']['median']:8.2f} ms  {r['B']} x DESC_init {r['b_init_single_calls_ms']['median']:9.2f} ms  "
          f"ratio {r['ratio_b_single_over_batch']:.2f}", flush=True)
    print(f"      (c) structure {c['ms_structure']['median']:.2f}  upload {c['ms_upload']['median']:.2f}  eig {c['ms_eig']['median']:.2f}  "
          f"project {c['ms_project']['median']:.2f}  total {c['ms_total']['median']:.2f} ms   |batch - single| {r['max_aligned_diff_batch_vs_single']:.1e}  "
          f"converged {r['converged']}", flush=True)
    if "d_streamed_call_ms" in r:
        print(f"      (d) streamed against lds: call {r['d_streamed_call_ms']['median']:.2f} / {r['d_lds_call_ms']['median']:.2f} ms "
              f"= {r['ratio_d_streamed_over_lds_call']:.2f}   eig {r['d_streamed_eig_ms']['median']:.2f} / {r['d_lds_eig_ms']['median']:.2f} ms "
              f"= {r['ratio_d_streamed_over_lds_eig']:.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="n:B, e.g. 100:64: measure this workload in this process and print its JSON row")
    ap.add_argument("--workloads", default=None, help="driver mode: n:B,n:B,... in place of the whole list, e.g. 400:16,748:16")
    ap.add_argument("--eig", choices=("lds", "streamed", "auto"), default="auto", help="the eigen-solve's mode in (a) to (c)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per workload (driver mode)")
    a = ap.parse_args()
    if a.only:
        n, B = (int(x) for x in a.only.split(":"))
        row = measure(n, B, a.reps, a.eig)
        show(row)
        print("ROW " + json.dumps(row), flush=True)
        return 0
    workloads = WORKLOADS if not a.workloads else [tuple(int(x) for x in w.split(":")) for w in a.workloads.split(",")]
    workloads = [(n, B) for n, B in workloads if a.eig != "lds" or n <= 278]
    rows = []
    for n, B in workloads:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--only", f"{n}:{B}", "--reps", str(a.reps),
               "--eig", a.eig]
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
            json.dump(dict(tool="tools/gcw_batch_stages.py", reps=a.reps, eig=a.eig, rows=rows), f, indent=1)
            f.write("\n")
    return 0 if len(rows) == len(workloads) else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""What the batched solver gains: one DESC_PGD_batch call against B consecutive DESC_PGD calls on the same arrays.

Workloads: B problems Uniform_Topology(100, 0.5, 0.2, 0.1) (the demo's size) and B problems of bench.py's C1 shape (n = 200), model
seeds 0 .. B-1, 100 iterations, lr = 0.01.  One process, one warm-up of each path, then the median and the spread (min .. max) of
`--reps` repetitions, synchronised host clock.  Per workload:
  (a) wall clock of one DESC_PGD_batch call;
  (b) wall clock of B consecutive DESC_PGD calls (the one-call path of the single solver);
  (c) the batch call's stages: structure / upload / cycle_d / pgd (desc_batch_result);
  (d) loop time per iteration and the batch's cycle count;
and once (e) the per-iteration time of the band sweep on one problem of similar total cycle count (C2).

--build host (the default), device or both: the builder of the batch's cycle structure (DESC_PGD_batch's ``build``).  With ``both`` the
two builders alternate inside every repetition of one process, next to the B consecutive calls, and every row carries (a), (c), (d)
and b/a per builder plus the device builder's per-kernel times; the S_vec of the two builders must be equal bit for bit.

    python tools/batch_stages.py [--reps 5] [--build both] [--out profiles/batch_structure_stages.json] [--only demo:64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from desc_amd import ConstantStepSize, DESC_PGD, DESC_PGD_batch, Uniform_Topology, _lib  # noqa: E402

SHAPES = {"demo": (100, (1, 16, 64, 256)), "C1": (200, (1, 16, 64))}
ITERS = 100


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


STAGES = ("ms_structure", "ms_upload", "ms_cycle_d", "ms_pgd", "ms_total")
LAPS = tuple("ms_build_" + k for k in _lib.Batch.BUILD_LAPS)


def measure(n, B, reps, builds=("host",)):
    models = [Uniform_Topology(n, 0.5, 0.2, 0.1, "uniform", seed=s) for s in range(B)]
    par = lambda: dict(iters=ITERS, Gradient=ConstantStepSize(0.01), seed=0, verbose=False)      # noqa: E731
    for bld in builds:
        DESC_PGD_batch(models, par(), build=bld)                                                 # warm-up (code objects, block caches)
    DESC_PGD(models[0].Ind, models[0].RijMat, par())
    ta = {b: [] for b in builds}; ta_plain = {b: [] for b in builds}; stages = {b: [] for b in builds}; S_b = {}
    tb, cycles, S_s = [], 0, None
    for _ in range(reps):
        for bld in builds:                                                                       # the builders alternate
            t0 = time.perf_counter()
            info = DESC_PGD_batch(models, par(), return_info=True, build=bld)
            ta[bld].append((time.perf_counter() - t0) * 1e3)
            assert info[0]["built_where"] == bld
            stages[bld].append(info[0]["timings"])
            cycles = int(sum(d["w"].size for d in info))
            S_b[bld] = [d["S_vec"] for d in info]
            # the plain (no return_info) batch call does not download w: timed separately as (a)
            t0 = time.perf_counter()
            DESC_PGD_batch(models, par(), build=bld)
            ta_plain[bld].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        S_s = [DESC_PGD(mo.Ind, mo.RijMat, par()) for mo in models]
        tb.append((time.perf_counter() - t0) * 1e3)
    for bld in builds[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(S_b[builds[0]], S_b[bld])), "the builders disagree"
    dev = max(float(np.abs(a - b).max()) for a, b in zip(S_b[builds[0]], S_s))

    def per_builder(bld):
        keys = STAGES + (LAPS if bld == "device" else ())
        return dict(a_batch_call_ms=stats(ta_plain[bld]), a_batch_call_with_info_ms=stats(ta[bld]),
                    ratio_b_over_a=float(np.median(tb) / np.median(ta_plain[bld])),
                    c_stages_ms={k: stats([s[k] for s in stages[bld]]) for k in keys},
                    d_loop_us_per_iteration=float(np.median([s["ms_pgd"] for s in stages[bld]]) / ITERS * 1e3))
    row = dict(n=n, B=B, iters=ITERS, m_cycle_total=cycles, b_consecutive_calls_ms=stats(tb), max_abs_diff_batch_vs_single=dev)
    row.update(per_builder(builds[0]))                   # the first builder's figures keep their places in the row
    row["build"] = builds[0]
    if len(builds) > 1:
        row["builders"] = {bld: per_builder(bld) for bld in builds}
    return row


def band_sweep_c2(reps):
    mo, nn, ii, jj, rij = bench.generate("C2")
    prob = _lib.ProblemArrays(nn, ii, jj, rij)
    st = _lib.Structure.build(prob, 30, 0, _lib.BUILD_HOST, 0)
    solver = _lib.Solver(prob, st, 0)
    st.free()
    try:
        p = _lib.default_params(); p.iters = ITERS * (reps + 1); p.lr = 0.01; p.stop_tol = -1.0
        solver.reset(p)
        solver.iterate_timed(ITERS)
        ms = [solver.iterate_timed(ITERS)[0] for _ in range(reps)]
        return dict(kernel=solver.kernel_name(), m_cycle=solver.m_cycle, us_per_iteration={k: v / ITERS * 1e3 for k, v in stats(ms).items()})
    finally:
        solver.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="shape:B, e.g. demo:64 (one workload, no C2 comparison)")
    ap.add_argument("--build", choices=("host", "device", "both"), default="host", help="the builder of the batch's cycle structure")
    a = ap.parse_args()
    builds = ("host", "device") if a.build == "both" else (a.build,)
    rows = []
    for name, (n, Bs) in SHAPES.items():
        for B in Bs:
            if a.only and a.only != f"{name}:{B}":
                continue
            row = measure(n, B, a.reps, builds)
            row["shape"] = name
            rows.append(row)
            c = row["c_stages_ms"]
            print(f"{name} n={n} B={B:4d}  cycles {row['m_cycle_total']:9d}  (a) batch {row['a_batch_call_ms']['median']:9.2f} ms "
                  f"[{row['a_batch_call_ms']['min']:.2f} .. {row['a_batch_call_ms']['max']:.2f}]  (b) {B} x DESC_PGD {row['b_consecutive_calls_ms']['median']:9.2f} ms "
                  f"[{row['b_consecutive_calls_ms']['min']:.2f} .. {row['b_consecutive_calls_ms']['max']:.2f}]  b/a {row['ratio_b_over_a']:.2f}", flush=True)
            print(f"      (c) structure {c['ms_structure']['median']:.2f}  upload {c['ms_upload']['median']:.2f}  cycle_d {c['ms_cycle_d']['median']:.2f}  "
                  f"pgd {c['ms_pgd']['median']:.2f} ms   (d) {row['d_loop_us_per_iteration']:.1f} us per iteration   "
                  f"|batch - single| {row['max_abs_diff_batch_vs_single']:.1e}", flush=True)
            for bld, r in row.get("builders", {}).items():
                c = r["c_stages_ms"]
                laps = "  ".join(f"{k[9:]} {c[k]['median']:.3f}" for k in LAPS if k in c)
                print(f"      build={bld:6s} (a) {r['a_batch_call_ms']['median']:9.2f} ms [{r['a_batch_call_ms']['min']:.2f} .. {r['a_batch_call_ms']['max']:.2f}]  "
                      f"b/a {r['ratio_b_over_a']:.2f}  structure {c['ms_structure']['median']:.2f}  upload {c['ms_upload']['median']:.2f}  "
                      f"cycle_d {c['ms_cycle_d']['median']:.2f}  pgd {c['ms_pgd']['median']:.2f}  {laps}", flush=True)
    out = dict(tool="tools/batch_stages.py", reps=a.reps, build=a.build, rows=rows)
    if not a.only:
        out["e_band_sweep_c2"] = band_sweep_c2(a.reps)
        e = out["e_band_sweep_c2"]
        print(f"(e) C2 single problem, {e['kernel']}: {e['m_cycle']} cycles, {e['us_per_iteration']['median']:.1f} us per iteration", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

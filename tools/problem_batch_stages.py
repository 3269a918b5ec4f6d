#!/usr/bin/env python3
"""What a resident ProblemBatch saves: the same batched calls on a list of problems and on the set made from them.

Workloads: n = 100 with B = 64 and 256, n = 200 with B = 64; problems of Uniform_Topology(n, 0.5, 0.2, 0.1) drawn on the GPU, model seeds
0 .. B-1; 100 PGD iterations (lr = 0.01).  Per workload, after one warm-up of each path, the median and the spread (min .. max) of
`--reps` repetitions of the host clock, the two paths taking turns inside every repetition:
  (a) the study, generator to score: Uniform_Topology_batch + DESC_batch(build="device") + Rotation_Alignment_batch on the models --
      the list path against the same three calls with resident=True;
  (b) a repeated solver call on problems that do not change: GCW_batch on the list against GCW_batch on a ProblemBatch made once
      (its one-time cost -- marshalling, CSR, upload -- is reported next to it, for either CSR builder);
  (c) the baseline curves on problems that do not change: CEMP_batch, CEMP_GCW_batch, CEMP_MST_batch, MPLS_batch and IRLS_GM_batch
      (the parameters of examples/monte_carlo.py) on the list against the same calls on a set drawn on the device
      (resident=True, made once): a time per call, and the bytes the set copied down over all of them (no rotation).
The byte counters stand next to the times: what the set copied up and down in (a), what the GCW handle's create uploaded in (b), and
what the list path's creates upload by the same counters, and what its generator's fetch copies back (161 bytes per edge, 72 per node);
in (c) what desc_cemp_batch_create_on, desc_irls_batch_create_on and desc_mst_batch_run_on move against the list path's creates.
The results of the two paths are compared bit for bit in every repetition.
Without --only the tool is a driver: every workload runs in a process of its own under its own time limit, and the first one that
fails ends the run.

    python tools/problem_batch_stages.py [--reps 5] [--out profiles/problem_batch_stages.json] [--workloads 100:64] [--only 100:64]
                                         [--timeout 240]
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

WORKLOADS = [(100, 64), (100, 256), (200, 64)]
ITERS = 100


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def same(a, b):
    """The results of two calls, lists and tuples of arrays, are the same in every bit."""
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def baselines():
    """Row (c)'s calls, by name: the curves of examples/monte_carlo.py that DESC is drawn against."""
    from desc_amd import CEMP_batch, CEMP_GCW_batch, CEMP_MST_batch, IRLS_GM_batch, MPLS_batch
    cemp = dict(max_iter=6, reweighting=[2.0 ** k for k in range(6)], nsample=50, seed=0)
    mpls = dict(stop_threshold=1e-3, max_iter=100, reweighting=cemp["reweighting"][-1], thresholding=[0.95, 0.9, 0.85, 0.8],
                cycle_info_ratio=1.0 / (np.arange(1, 101) + 1))
    return dict(CEMP_batch=lambda p: CEMP_batch(p, cemp), CEMP_GCW_batch=lambda p: CEMP_GCW_batch(p, cemp),
                CEMP_MST_batch=lambda p: CEMP_MST_batch(p, cemp), MPLS_batch=lambda p: MPLS_batch(p, cemp, mpls),
                IRLS_GM_batch=lambda p: IRLS_GM_batch(p)), cemp


def measure(n, B, reps):
    from desc_amd import ConstantStepSize, DESC_batch, DESC_PGD_batch, GCW_batch, ProblemBatch, Rotation_Alignment_batch, Uniform_Topology_batch, _lib
    par = lambda: dict(iters=ITERS, Gradient=ConstantStepSize(0.01), seed=0, verbose=False)      # noqa: E731
    seeds = list(range(B))

    def study(resident):
        models = Uniform_Topology_batch(n, 0.5, 0.2, 0.1, "uniform", seeds=seeds, resident=resident)
        out = DESC_batch(models, par(), build="device")
        score = Rotation_Alignment_batch([R for R, _, _ in out], models, rotations=False)
        moved = models.bytes() if resident else None
        if resident:
            models.close()
        return out, score, moved

    models = Uniform_Topology_batch(n, 0.5, 0.2, 0.1, "uniform", seeds=seeds)
    M = int(sum(mo.Ind.shape[0] for mo in models))
    S = DESC_PGD_batch(models, par())
    sets, t_set = {}, dict(host=[], device=[])
    for csr in ("host", "device"):                                                               # warm-up of the set's create, then timed
        ProblemBatch(models, csr=csr).close()
    study(False); study(True); GCW_batch(models, S)                                              # warm-up (code objects, block caches)
    calls, cemp = baselines()
    drawn = Uniform_Topology_batch(n, 0.5, 0.2, 0.1, "uniform", seeds=seeds, resident=True)     # row (c)'s set: made once, never fetched
    drawn_bytes = drawn.bytes()
    for call in calls.values():
        call(models); call(drawn)
    t_c = {name: dict(list=[], set=[]) for name in calls}
    t = dict(a_list=[], a_resident=[], b_list=[], b_set=[])
    moved_a = moved_b = None
    for _ in range(reps):
        for csr in ("host", "device"):
            if csr in sets:
                sets[csr].close()
            sets[csr], ms = clock(lambda: ProblemBatch(models, csr=csr))
            t_set[csr].append(ms)
        (out_l, score_l, _), ms = clock(lambda: study(False)); t["a_list"].append(ms)
        (out_r, score_r, moved_a), ms = clock(lambda: study(True)); t["a_resident"].append(ms)
        assert all(np.array_equal(x, y) for a, b in zip(out_l, out_r) for x, y in zip(a, b))     # the same bits from either path
        assert all(a[2] == b[2] and a[3] == b[3] for a, b in zip(score_l, score_r))
        R_l, ms = clock(lambda: GCW_batch(models, S)); t["b_list"].append(ms)
        R_s, ms = clock(lambda: GCW_batch(sets["device"], S)); t["b_set"].append(ms)
        assert all(np.array_equal(x, y) for x, y in zip(R_l, R_s))
        for name, call in calls.items():
            out_l, ms = clock(lambda: call(models)); t_c[name]["list"].append(ms)
            out_s, ms = clock(lambda: call(drawn)); t_c[name]["set"].append(ms)
            assert same(out_l, out_s), name
    h = _lib.GcwBatch(None, on=sets["device"]._set)
    moved_b = h.bytes()
    h.destroy()
    # what the list path's three creates upload, by the same counters
    from desc_amd.algorithms import _marshal_problems, make_c_params
    probs, _ = _marshal_problems(models)
    list_up = {}
    for name, make in (("gcw", lambda: _lib.GcwBatch(probs)), ("refine", lambda: _lib.RefineBatch(probs)),
                       ("pgd", lambda: _lib.Batch(probs, make_c_params(par())[0], where=_lib.BUILD_DEVICE))):
        h = make()
        list_up[name] = h.bytes()[0]
        h.destroy()
    # row (c): what the creates on the drawn set move, and the list path's creates by the same counters
    c_bytes = {}
    for name, on_set, on_list in (("cemp", lambda: _lib.CempBatch(None, cemp["nsample"], on=drawn._set), lambda: _lib.CempBatch(probs, cemp["nsample"])),
                                  ("irls", lambda: _lib.IrlsBatch(None, None, on=drawn._set), lambda: _lib.IrlsBatch(probs))):
        hs, hl = on_set(), on_list()
        c_bytes[name] = dict(on_set=dict(zip(("h2d", "d2h"), hs.bytes())), on_list=dict(zip(("h2d", "d2h"), hl.bytes())))
        hs.destroy(); hl.destroy()
    moved = _lib.mst_batch_run_on(drawn._set, np.full(M, 0.5), return_bytes=True)[2]
    c_bytes["mst"] = dict(on_set=dict(h2d=moved[0], d2h=moved[1]), on_list=dict(h2d=24 * M + 4 * (n * B + B) + 16 * B, d2h=4 * n * B))     # the list's: S_vec and its CSR, by size
    drawn_after = drawn.bytes()
    drawn.close()
    set_bytes = {csr: sets[csr].bytes() for csr in sets}
    for s in sets.values():
        s.close()
    return dict(n=n, B=B, iters=ITERS, edges=M,
                a_list_ms=stats(t["a_list"]), a_resident_ms=stats(t["a_resident"]),
                ratio_a_list_over_resident=float(np.median(t["a_list"]) / np.median(t["a_resident"])),
                a_resident_set_bytes=dict(h2d=moved_a[0], d2h=moved_a[1]), a_list_bytes=dict(h2d=sum(list_up.values()), d2h=161 * M + 72 * n * B),
                b_list_ms=stats(t["b_list"]), b_set_ms=stats(t["b_set"]),
                ratio_b_list_over_set=float(np.median(t["b_list"]) / np.median(t["b_set"])),
                b_create_on_bytes=dict(h2d=moved_b[0], d2h=moved_b[1]), b_list_create_bytes=dict(h2d=list_up["gcw"]),
                c_ms={name: dict(list=stats(v["list"]), set=stats(v["set"]), ratio_list_over_set=float(np.median(v["list"]) / np.median(v["set"])))
                      for name, v in t_c.items()},
                c_bytes=c_bytes, c_set_d2h=dict(at_creation=drawn_bytes[1], after_all_calls=drawn_after[1]),
                set_create_ms={csr: stats(v) for csr, v in t_set.items()},
                set_create_bytes={csr: dict(h2d=v[0], d2h=v[1]) for csr, v in set_bytes.items()})


def show(r):
    a, b = r["a_list_ms"], r["a_resident_ms"]
    print(f"n={r['n']} B={r['B']:4d} ({r['edges']} edges)  (a) generator + DESC_batch(device) + scoring: list {a['median']:8.2f} ms "
          f"[{a['min']:.2f} .. {a['max']:.2f}]  resident {b['median']:8.2f} ms [{b['min']:.2f} .. {b['max']:.2f}]  "
          f"ratio {r['ratio_a_list_over_resident']:.2f}", flush=True)
    print(f"      bytes: the resident set copied {r['a_resident_set_bytes']['h2d']} up, {r['a_resident_set_bytes']['d2h']} down; the list path's "
          f"three creates {r['a_list_bytes']['h2d']} up, its generator's fetch {r['a_list_bytes']['d2h']} down", flush=True)
    a, b = r["b_list_ms"], r["b_set_ms"]
    print(f"      (b) GCW_batch repeated: on the list {a['median']:8.2f} ms [{a['min']:.2f} .. {a['max']:.2f}]  on the set {b['median']:8.2f} ms "
          f"[{b['min']:.2f} .. {b['max']:.2f}]  ratio {r['ratio_b_list_over_set']:.2f}   create_on uploads {r['b_create_on_bytes']['h2d']} B, "
          f"the list's create {r['b_list_create_bytes']['h2d']} B", flush=True)
    for name, v in r.get("c_ms", {}).items():
        print(f"      (c) {name:15s} on the list {v['list']['median']:8.2f} ms [{v['list']['min']:.2f} .. {v['list']['max']:.2f}]  on the drawn set "
              f"{v['set']['median']:8.2f} ms [{v['set']['min']:.2f} .. {v['set']['max']:.2f}]  ratio {v['ratio_list_over_set']:.2f}", flush=True)
    if "c_bytes" in r:
        cb, d = r["c_bytes"], r["c_set_d2h"]
        print("      (c) bytes up / down: " + ";  ".join(f"{k} on the set {v['on_set']['h2d']} / {v['on_set']['d2h']}, on the list "
                                                          f"{v['on_list']['h2d']} / {v['on_list']['d2h']}" for k, v in cb.items()), flush=True)
        print(f"      (c) the drawn set copied down {d['at_creation']} bytes at creation and {d['after_all_calls']} after every call", flush=True)
    c = r["set_create_ms"]
    print(f"      the set, once: ProblemBatch(csr='host') {c['host']['median']:.2f} ms, csr='device' {c['device']['median']:.2f} ms "
          f"({r['set_create_bytes']['host']['h2d']} / {r['set_create_bytes']['device']['h2d']} bytes up)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="n:B, e.g. 100:64: measure this workload in this process and print its JSON row")
    ap.add_argument("--workloads", default=None, help="driver mode: n:B,n:B,... in place of the whole list")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per workload (driver mode)")
    a = ap.parse_args()
    if a.only:
        n, B = (int(x) for x in a.only.split(":"))
        row = measure(n, B, a.reps)
        show(row)
        print("ROW " + json.dumps(row), flush=True)
        return 0
    workloads = WORKLOADS if not a.workloads else [tuple(int(x) for x in w.split(":")) for w in a.workloads.split(",")]
    rows = []
    for n, B in workloads:
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
            json.dump(dict(tool="tools/problem_batch_stages.py", reps=a.reps, rows=rows), f, indent=1)
            f.write("\n")
    return 0 if len(rows) == len(workloads) else 1


if __name__ == "__main__":
    sys.exit(main())

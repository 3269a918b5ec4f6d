#!/usr/bin/env python3
"""bench.py -- DESC_PGD iterations/second on MI355X (BASELINE.json metric).

A "step" is one PGD iteration (one sweep over all sampled 3-cycles: mirror sums,
gradient, tangent projection, step, per-edge simplex projection, new S_vec) on a
synthetic Uniform_Topology graph whose structure, rotations and cycle
inconsistencies are already resident in HBM when the timed region starts.

    python bench.py --gpus N --steps K --warmup W [--workload C1..C5] [--dump-outputs DIR] [--full]

`value` is BASELINE.json configs[3] (C4: Uniform n=5000 p=0.2 q=0.3 sigma=0.1 -- the workload the north star's
target is quoted on; 4 GB, fits one GPU) at every N: strong scaling, the total work is fixed, at N > 1 the
edges-with-cycles are sharded over the ranks with a reduce-scatter and an all-gather per iteration
(desc_amd/sharded.py).

A plain run sets up, warms up, times the K steps and prints the line; `--dump-outputs DIR` also writes what the
last timed step left (S_vec and the objective / average-change traces, float64) as DIR/<name>.npy.  Everything
else is measured under `--full` only: the per-kernel `roofline` leg (dominant kernels: column sums + sweep,
HBM-bound, algorithmic bytes 72*m_cycle + 12*m_pos per iteration), the timed `end_to_end` solve
calls, the run to the patience exit, `cpu_baseline` (the oracle's OpenMP C restatement timed on this host for a
bounded number of iterations of the same workload; rank 0) with `parity_vs_cpu`, and `secondary_config`: the
same measurement on C2 (configs[1], n=1000 p=0.5).

`--gpus N` without WORLD_SIZE in the environment starts the N ranks itself (one child process per GPU, before
anything in this process touches a GPU); under `python -m torch.distributed.run` the ranks are already there.
Rank 0 prints ONE JSON line with the contract's fields, at N > 1 with `rccl_ranks` (ncclCommCount of the
communicator the collectives ran on).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

WORKLOADS = {
    # name: (generator kwargs, description)
    "C1": dict(kind="uniform", n=200, p=0.5, q=0.2, sigma=0.1, model="uniform", seed=0),
    "C2": dict(kind="uniform", n=1000, p=0.5, q=0.3, sigma=0.1, model="uniform", seed=1),
    "C3": dict(kind="nonuniform", n=2000, p=0.2, p_node_crpt=0.5, p_edge_crpt=0.5, sigma_in=0.1, sigma_out=0.1,
               crpt_type="self-consistent", seed=2),
    "C4": dict(kind="uniform", n=5000, p=0.2, q=0.3, sigma=0.1, model="uniform", seed=3),
    "C5": dict(kind="uniform", n=10000, p=0.1, q=0.3, sigma=0.1, model="uniform", seed=4),
}
HBM_PEAK_GBS = 8000.0     # MI355X spec, /opt/skills/guides/MI355X_MICROARCH.md
HBM_COPY_GBS = 6290.0     # measured device-to-device copy rate, same guide: what a kernel that only streams can reach


def describe(name):
    w = WORKLOADS[name]
    if w["kind"] == "uniform":
        return (f"{name}: Uniform_Topology n={w['n']} p={w['p']} q={w['q']} sigma={w['sigma']} '{w['model']}' "
                f"seed={w['seed']}; DESC_PGD ConstantStepSize(0.01)")
    return (f"{name}: Nonuniform_Topology n={w['n']} p={w['p']} p_node_crpt={w['p_node_crpt']} "
            f"p_edge_crpt={w['p_edge_crpt']} sigma_in={w['sigma_in']} sigma_out={w['sigma_out']} "
            f"'{w['crpt_type']}' seed={w['seed']}; DESC_PGD ConstantStepSize(0.01)")


def generate(name):
    from desc_amd.algorithms import marshal_edges
    from desc_amd.models import Nonuniform_Topology, Uniform_Topology
    w = dict(WORKLOADS[name])
    kind = w.pop("kind")
    if kind == "uniform":
        mo = Uniform_Topology(w["n"], w["p"], w["q"], w["sigma"], w["model"], seed=w["seed"])
    else:
        mo = Nonuniform_Topology(w["n"], w["p"], w["p_node_crpt"], w["p_edge_crpt"], w["sigma_in"], w["sigma_out"],
                                 w["crpt_type"], seed=w["seed"])
    nn, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    return mo, nn, ii, jj, rij


def cpu_baseline(nn, ii, jj, rij, arrays, budget_s=20.0, max_iters=50, threads=None):
    """Time the oracle's C/OpenMP restatement of the same sweep on this host (threads=None: every CPU granted to this process --
    affinity mask cut down by the cgroup quota, oracle.granted_cpus()).  Also returns the oracle's result: main() compares the GPU's
    S_vec after the same number of iterations with it (`parity_vs_cpu`)."""
    from oracle import oracle as O
    O.build()
    L = O.lib()
    default_threads = O.num_threads()
    if threads:
        L.oracle_set_threads(int(threads))
    try:
        st = {k: arrays[k] for k in ("m", "m_pos", "m_cycle", "pos_edge", "cum_ind", "k", "e_jk", "e_ki", "ikj", "jki")}
        S0 = O.cycle_d(ii, jj, rij.reshape(-1, 9), st)
        t = time.perf_counter()
        O.pgd_run(st, S0, 2, lr=0.01, patience=1 << 30)
        per_iter = (time.perf_counter() - t) / 2
        iters = int(max(2, min(max_iters, budget_s / max(per_iter, 1e-6))))
        t = time.perf_counter()
        ref = O.pgd_run(st, S0, iters, lr=0.01, patience=1 << 30)
        dt = time.perf_counter() - t
        cores = O.num_threads()
    finally:
        L.oracle_set_threads(default_threads)
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            model = next((ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")), "")
    except OSError:
        pass
    g = O.granted_cpus()
    return dict(value=iters / dt, unit="iters/s", cores=cores, kind="port",
                sample=f"{iters} PGD iterations of the same workload (oracle/desc_oracle.c, OpenMP)",
                cpus_granted=g["granted"], cpus_in_affinity_mask=g["affinity"], cgroup_cpu_quota=g["cgroup_quota"],
                host_cpus=os.cpu_count(), cpu_model=model), ref, iters


def parity_vs_cpu(lib, prob, ref, iters, seed, n_sample_min=30):
    """The north star's acceptance figure, stated: mean / max |S_vec(GPU) - S_vec(CPU oracle)| after the same `iters` iterations
    of the same workload on the same cycle structure (the oracle ran on the structure the GPU built; one desc_pgd_solve call
    rebuilds it from the same seed).  BASELINE.md plan item 4; SURVEY.md 8c bound: max <= 1e-10."""
    p = lib.default_params()
    p.iters = iters; p.lr = 0.01; p.seed = seed; p.patience = (1 << 31) - 1; p.n_sample_min = n_sample_min
    out = lib.solve(prob, p)
    d = np.abs(out["S_vec"] - ref["S_vec"])
    do = np.abs(out["obj"] - ref["obj"][:out["iters_run"]]) / np.maximum(np.abs(ref["obj"][:out["iters_run"]]), 1e-300)
    return {"iters": int(iters), "mean_abs": float(d.mean()), "max_abs": float(d.max()), "objective_max_rel": float(do.max()),
            "what": "S_vec of the HIP path vs oracle/desc_oracle.c (OpenMP) after the same iterations, same structure",
            "north_star_bound_mean_abs": 1e-6, "test_bound_max_abs": 1e-10}


def literal_baseline(budget_iters=4):
    """SURVEY.md 8d "reference-style interpreted" data point: the line-by-line NumPy restatement of DESC_PGD.m
    (dense n x n / n x m_pos arrays, interpreted per-edge loops, like the MATLAB original) on C1, the only
    BASELINE configuration the reference's own data structures fit comfortably."""
    from oracle.desc_pgd_literal import ConstantStepSize as LConst, desc_pgd_literal
    from oracle.oracle import keyed_sampler
    mo, nn, ii, jj, rij = generate("C1")
    t = time.perf_counter()
    desc_pgd_literal(mo.Ind, mo.RijMat, 0, LConst(0.01), sampler=keyed_sampler(0))
    t_setup = time.perf_counter() - t
    t = time.perf_counter()
    desc_pgd_literal(mo.Ind, mo.RijMat, budget_iters, LConst(0.01), sampler=keyed_sampler(0))
    t_run = time.perf_counter() - t
    per_iter = max(t_run - t_setup, 1e-9) / budget_iters
    return dict(value=1.0 / per_iter, unit="iters/s", cores=1, kind="port",
                sample=f"{budget_iters} iterations of oracle/desc_pgd_literal.py (interpreted NumPy, dense arrays) on {describe('C1')}",
                setup_s=t_setup)


def warm_up(lib):
    """One call on a 200-node complete graph, outside every timer: HIP context, code-object load, the runtime's
    pinned staging buffers and first-use kernel attributes are per-process one-time costs."""
    wi, wj = np.triu_indices(200, 1)
    wprob = lib.ProblemArrays(200, wi.astype(np.int32), wj.astype(np.int32), np.tile(np.eye(3).reshape(-1), wi.shape[0]))
    wp = lib.default_params(); wp.iters = 2
    lib.solve(wprob, wp)


def load_traffic(name):
    """HBM bytes per iteration from the PMC passes committed under profiles/ (rocprofv3 cannot run inside the
    bench): FETCH_SIZE and WRITE_SIZE collected in separate runs, corrected as MI355X_MICROARCH.md prescribes
    (tools/pmc_traffic.py); null for workloads that have not been profiled."""
    for fn in ("r04_traffic.json", "r03_traffic.json", "r02_traffic.json", "r01_traffic.json"):
        try:
            with open(os.path.join(ROOT, "profiles", fn)) as f:
                t = json.load(f).get(name, {}).get("per_iteration_bytes")
            if t:
                return t, fn
        except OSError:
            pass
    return None, None


def measure(lib, name, K, W, seed, n_sample_min=30, full=False, convergence=False, keep_arrays=False, want_outputs=False):
    """One workload on one GPU: K timed iterations (inputs resident in HBM); with want_outputs, what the last of them left
    (`outputs`: the arrays Solver.download hands a caller).  full: also the per-kernel roofline leg, one really timed
    desc_pgd_solve call (host arrays in -> S_vec out, 100 iterations), optionally the run to the patience exit."""
    t0 = time.perf_counter()
    mo, nn, ii, jj, rij = generate(name)
    t_gen = time.perf_counter() - t0
    prob = lib.ProblemArrays(nn, ii, jj, rij)
    t0 = time.perf_counter()
    st = lib.Structure.build(prob, n_sample_min, seed, lib.BUILD_DEVICE, 0)
    t_struct = time.perf_counter() - t0
    t0 = time.perf_counter()
    solver = lib.Solver(prob, st, 0)
    t_create = time.perf_counter() - t0
    sizes = st.sizes()
    arrays = st.arrays() if keep_arrays else None     # host copy for the CPU baseline only (untimed; the GPU path never needs it)
    st.free()

    p = lib.default_params()
    p.iters = W + 2 * K + 8
    p.lr = 0.01
    p.patience = (1 << 31) - 1          # the bench times exactly K sweeps: never stop early
    p.seed = seed
    solver.reset(p)
    solver.iterate(W)
    solver.sync()
    # ---- timed region: exactly K steps, inputs resident in HBM ----
    t0 = time.perf_counter()
    solver.iterate(K)
    solver.sync()
    dt = time.perf_counter() - t0
    # taken before anything else runs on the handle, so a plain run and a --full run write the same arrays
    outputs = solver.download() if want_outputs else None
    m_cycle, m_pos, m = solver.m_cycle, solver.m_pos, solver.m
    res = dict(name=name, nn=nn, m=m, m_pos=m_pos, m_cycle=m_cycle, n_sample=int(sizes["n_sample"]), dt=dt, outputs=outputs,
               setup_ms={"generate": t_gen * 1e3, "structure_device": t_struct * 1e3, "upload_layout_cycle_d": t_create * 1e3})
    if not full:
        solver.destroy()
        return res
    # ---- roofline leg: the same K sweeps again, each iteration's kernels bracketed by HIP events
    #      on the launch stream (not part of `value`) ----
    _, ms_kernel = solver.iterate_timed(K, per_kernel=True)
    out = solver.download()
    kname = solver.kernel_name()
    lay = solver.layout_stats()
    conv = None
    if convergence:
        # wall-clock to the reference's own stopping rule (DESC_PGD.m:243-256: objective decrease < 1e-5 for 30
        # consecutive iterations), reached with ConstantStepSize(1); not part of `value`
        pc = lib.default_params()
        pc.iters = 5000; pc.lr = 1.0; pc.seed = seed
        t0 = time.perf_counter()
        conv = solver.run(pc)
        conv["t"] = time.perf_counter() - t0
    solver.destroy()
    # ---- end to end, really timed: one desc_pgd_solve call = structure build + upload + layout + S0_long +
    #      100 iterations + download (what DESC_PGD() / the MEX shim pay per call in a warm process)
    pe = lib.default_params(); pe.iters = 100; pe.lr = 0.01; pe.seed = seed; pe.patience = (1 << 31) - 1; pe.n_sample_min = n_sample_min
    lib.trim_memory()                   # the blocks parked by the handle above go back to the driver: this call allocates afresh
    t0 = time.perf_counter()
    e2e = lib.solve(prob, pe)
    t_e2e = time.perf_counter() - t0
    # ... and the same call again: device and host blocks parked by the first one are reused (every later call of a session)
    t_e2e_again = None
    for _ in range(2):                  # best of two: single calls scatter by +-10 % on a shared host
        t0 = time.perf_counter()
        x = lib.solve(prob, pe)
        dt_x = time.perf_counter() - t0
        if t_e2e_again is None or dt_x < t_e2e_again:
            t_e2e_again, e2e_again = dt_x, x

    bytes_per_launch = 72.0 * m_cycle + 12.0 * m_pos
    achieved = bytes_per_launch / (ms_kernel * 1e-3) / 1e9 if ms_kernel else 0.0
    traffic, traffic_src = load_traffic(name)
    # What THIS layout has to stream per iteration at the very least: the sweep's 28 bytes per cycle (old and new
    # weight, S0, packed word), the column sums' 10 bytes per (cycle, endpoint) whose mirror was sampled (weight + 16-bit column index),
    # 12 bytes per segment (record + new S).  The 72-byte count above prices four 8-byte gathers per cycle that the band layout serves from
    # the LDS and the caches: on graphs that fit the caches `frac` can therefore exceed 1 -- it is the contract's figure, not an HBM fraction.
    node_layout = any(x in kname for x in ("node", "band", "small"))
    floor_bytes = 28.0 * m_cycle + 10.0 * lay.get("colsum_entries", 0) + 12.0 * m_pos if node_layout else bytes_per_launch
    sec = ms_kernel * 1e-3 if ms_kernel else float("inf")
    res.update(
        mo=mo, ii=ii, jj=jj, rij=rij, prob=prob, arrays=arrays, out=out,
        roofline={"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                  "traffic": traffic, "traffic_source": traffic_src,
                  "frac_traffic": (traffic / sec / 1e9 / HBM_PEAK_GBS) if traffic else None,
                  "frac_of_copy_peak": (traffic / sec / 1e9 / HBM_COPY_GBS) if traffic else None, "copy_peak": HBM_COPY_GBS,
                  "floor_bytes": floor_bytes, "floor_ms_at_copy_peak": floor_bytes / (HBM_COPY_GBS * 1e9) * 1e3,
                  "note": "frac = 72-byte algorithmic count / kernel time / 8 TB/s (the contract's figure; it prices gathers the band layout serves "
                          "from LDS and caches, so it can exceed 1 on cache-resident graphs); frac_traffic = PMC-measured HBM bytes over the same time",
                  "layout": lay,
                  "kernel": ("k_colsum_node + " + kname + "0> (one iteration = both launches)") if node_layout else kname,
                  "bytes_per_launch": bytes_per_launch, "kernel_ms": ms_kernel},
        end_to_end={"ms": t_e2e * 1e3, "what": "one timed desc_pgd_solve call: host arrays in -> S_vec out, 100 iterations, warm HIP context, every block allocated afresh",
                    "ms_structure": e2e["ms_structure"], "ms_upload": e2e["ms_upload"], "ms_layout_cycle_d": e2e["ms_cycle_d"],
                    "ms_pgd": e2e["ms_pgd"], "ms_total_in_library": e2e["ms_total"],
                    "repeat_ms": t_e2e_again * 1e3, "repeat_what": "the same call again (best of two): the blocks the first call released are reused (devmem.hip / hostmem.h)",
                    "repeat_ms_structure": e2e_again["ms_structure"], "repeat_ms_pgd": e2e_again["ms_pgd"]},
        conv=None if conv is None else
        {"iters_run": int(conv["iters_run"]), "ms_iterations": conv["t"] * 1e3,
         "mean_abs_err_vs_truth": float(np.mean(np.abs(conv["S_vec"] - mo.ErrVec)))},
        err=float(np.mean(np.abs(out["S_vec"] - mo.ErrVec))))
    return res


def dump_outputs(directory, outputs):
    """--dump-outputs: the arrays the timed path hands a caller after its last step, float64.  Whole, not sampled: S_vec has
    m entries, at most ~5e6 (C5: 40 MB)."""
    arrays = {"S_vec": outputs["S_vec"], "obj": outputs["obj"], "avg": outputs["avg"]}
    total = sum(a.nbytes for a in arrays.values())
    if total > 64 << 20:
        raise RuntimeError(f"--dump-outputs: {total} bytes exceed the 64 MB the outputs may take")
    os.makedirs(directory, exist_ok=True)
    for key, a in arrays.items():
        np.save(os.path.join(directory, key + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def spawn_ranks(args, argv):
    """`bench.py --gpus N` started as ONE process: start N ranks of this script (RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* in their environment, one GPU each), before anything in this process has touched a GPU; rank 0 prints the
    JSON line.  Non-zero exit if any rank fails (the others are stopped by PID)."""
    import subprocess
    env = dict(os.environ, WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    procs = []
    for r in range(args.gpus):
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv,
                                      env=dict(env, RANK=str(r), LOCAL_RANK=str(r))))
    rc = 0
    pending = list(procs)
    while pending:
        for q in list(pending):
            code = q.poll()
            if code is None:
                continue
            pending.remove(q)
            if code != 0 and rc == 0:
                rc = code
                for other in pending:              # a rank died: the rest would wait in a collective for ever
                    other.terminate()
        time.sleep(0.05)
    return rc


def dry_launch(args):
    """Launch rehearsal without a GPU (tests): the ranks meet over gloo, count themselves, rank 0 prints what it saw."""
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t = torch.ones(1, dtype=torch.int64)
    dist.all_reduce(t)
    seen = int(t.item())
    # the hand-over of the synthetic problem (rank 0 generates, the others map its arrays): every rank must end up with the same bytes,
    # and only rank 0 may have run the generator
    from desc_amd.sharded import TorchComm, shared_problem
    calls = []

    def gen(name):
        calls.append(name)
        return generate(name)

    nn, ii, jj, rij, err = shared_problem("C1", rank, world, TorchComm(), gen)
    digest = torch.tensor([float(nn), float(ii.sum()), float(jj.sum()), float(np.abs(rij).sum()), float(err.sum())], dtype=torch.float64)
    lo, hi = digest.clone(), digest.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    ncalls = torch.tensor([len(calls)], dtype=torch.int64)
    dist.all_reduce(ncalls)
    shared_ok = bool(torch.equal(lo, hi)) and int(ncalls.item()) == 1 and len(calls) == (1 if rank == 0 else 0)
    ok = seen == args.gpus == world and shared_ok
    if rank == 0:
        print(json.dumps({"dry_launch": True, "n_gpus": world, "ranks_counted": seen, "requested": args.gpus, "problem_shared": shared_ok,
                          "generator_calls": int(ncalls.item()), "ok": ok}), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    return 0 if ok else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true", help="measure everything beyond the headline as well: roofline leg, timed end-to-end "
                    "solve calls, run to the patience exit, CPU baseline with parity, and C2 as secondary_config")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step left (S_vec, obj, avg; "
                    "float64) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-convergence", action="store_true", help="--full without the run to the patience exit")
    ap.add_argument("--no-secondary", "--no-north-star", dest="no_secondary", action="store_true", help="--full without the extra C2 measurement")
    ap.add_argument("--seed", type=int, default=0, help="cycle-sampling seed")
    ap.add_argument("--all-triangles", action="store_true", help="no cycle sampling: n_sample_min above every codegree, all triangles swept "
                    "(BASELINE configs[4]: ~1.7e8 triangles = 5e8 edge-cycle slots at C5)")
    ap.add_argument("--dry-launch", action="store_true", help="start the ranks, let them count themselves over gloo, touch no GPU (launch test)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_ranks(args, sys.argv[1:])             # nothing above or in here initialises a GPU
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.dry_launch:
        return dry_launch(args)
    if world != args.gpus and not (world == 1 and args.gpus == 1):
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a line for the wrong rank count", file=sys.stderr)
        return 2
    if world > 1 or os.environ.get("DESC_FORCE_SHARDED") == "1":   # the env switch rehearses the N>1 code path on one GPU
        if args.dump_outputs:
            print("bench.py: --dump-outputs is not implemented for the sharded path", file=sys.stderr)
            return 2
        if not args.full:
            args.no_secondary = args.no_cpu_baseline = True
        from desc_amd.sharded import bench_sharded
        return bench_sharded(args, WORKLOADS, describe, generate, cpu_baseline)

    from desc_amd import _lib
    name = args.workload or "C4"
    K, W = args.steps, args.warmup
    warm_up(_lib)
    nsm = (1 << 16) if args.all_triangles else 30
    # (unsampled: ConstantStepSize(1) never meets the patience rule -- 5000 sweeps measured at C5 -- so that leg is skipped)
    r = measure(_lib, name, K, W, args.seed, nsm, full=args.full, convergence=not args.no_convergence and not args.all_triangles,
                keep_arrays=args.full and not args.no_cpu_baseline, want_outputs=args.dump_outputs is not None)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, r["outputs"])
    dt = r["dt"]
    line = {
        "metric": "DESC_PGD iters/sec", "value": K / dt, "unit": "iters/s", "n_gpus": 1, "steps": K, "warmup": W,
        "ms_per_step": dt / K * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": describe(name) + ("; all triangles (no cycle sampling)" if args.all_triangles else ""), "n": r["nn"], "m": r["m"], "m_pos": r["m_pos"], "m_cycle": r["m_cycle"],
                   "n_sample": r["n_sample"], "sampling_seed": args.seed, "parallelism": "1 GPU"},
        "cycle_updates_per_s": r["m_cycle"] * K / dt,
        "setup_ms": r["setup_ms"],
    }
    if not args.full:
        print(json.dumps(line))
        return 0
    line.update({
        "roofline": r["roofline"],
        "end_to_end_100_iters_ms": r["end_to_end"]["ms"],
        "end_to_end": r["end_to_end"],
        "to_patience_exit_lr1": r["conv"],
        "mean_abs_err_vs_truth": r["err"],
    })
    if not args.no_cpu_baseline:
        # the oracle's C/OpenMP port on the same workload, a bounded number of iterations (C4: ~0.5 s each on 16 threads)
        cb, ref, it = cpu_baseline(r["nn"], r["ii"], r["jj"], r["rij"], r["arrays"], budget_s=12.0, max_iters=10 if name in ("C4", "C5") else 50)
        line["cpu_baseline"] = cb
        line["gpu_over_cpu"] = line["value"] / cb["value"]
        line["parity_vs_cpu"] = parity_vs_cpu(_lib, r["prob"], ref, it, args.seed, nsm)
        r["arrays"] = None
    else:
        line["cpu_baseline"] = None
    if args.workload is None and not args.no_secondary:
        # BASELINE configs[1] (C2, n=1000 p=0.5): same measurement, its own roofline and CPU data points
        x = measure(_lib, "C2", K, W, args.seed, full=True, convergence=not args.no_convergence, keep_arrays=not args.no_cpu_baseline)
        sec = {"workload": describe("C2"), "value": K / x["dt"], "unit": "iters/s", "steps": K, "warmup": W, "ms_per_step": x["dt"] / K * 1e3,
               "m_cycle": x["m_cycle"], "m_pos": x["m_pos"], "n_sample": x["n_sample"], "roofline": x["roofline"],
               "setup_ms": x["setup_ms"], "end_to_end": x["end_to_end"], "to_patience_exit_lr1": x["conv"], "mean_abs_err_vs_truth": x["err"]}
        if not args.no_cpu_baseline:
            cb2, ref2, it2 = cpu_baseline(x["nn"], x["ii"], x["jj"], x["rij"], x["arrays"], budget_s=6.0, max_iters=50)
            sec["cpu_baseline"] = cb2
            sec["gpu_over_cpu"] = sec["value"] / cb2["value"]
            sec["parity_vs_cpu"] = parity_vs_cpu(_lib, x["prob"], ref2, it2, args.seed)
            # SURVEY.md 8d's other two data points (reported, never the target): the same port on one thread, and
            # the interpreted literal restatement on C1
            one, _, _ = cpu_baseline(x["nn"], x["ii"], x["jj"], x["rij"], x["arrays"], budget_s=5.0, max_iters=6, threads=1)
            variants = {"port_single_thread_C2": one}
            try:
                variants["literal_numpy_C1"] = literal_baseline()
            except Exception as e:            # the literal restatement is test infrastructure: never fail the bench on it
                variants["literal_numpy_C1"] = {"error": repr(e)}
            line["cpu_baseline_variants"] = variants
        line["secondary_config"] = sec
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

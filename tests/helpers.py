"""Shared helpers for the parity tests."""
import numpy as np

from desc_amd import _lib
from desc_amd.algorithms import marshal_edges
from desc_amd.models import Nonuniform_Topology, Uniform_Topology


def make_problem(kind="uniform", n=60, p=0.5, q=0.2, sigma=0.1, seed=0, **kw):
    if kind == "uniform":
        mo = Uniform_Topology(n, p, q, sigma, kw.get("model", "uniform"), seed=seed)
    else:
        mo = Nonuniform_Topology(n, p, kw.get("p_node_crpt", 0.5), kw.get("p_edge_crpt", 0.5),
                                 kw.get("sigma_in", 0.1), kw.get("sigma_out", 0.1),
                                 kw.get("crpt_type", "self-consistent"), seed=seed)
    nn, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None
    return mo, nn, ii, jj, rij


def oracle_reference(O, nn, ii, jj, rij, seed, iters, **step):
    st = O.build_structure(nn, ii, jj, seed=seed)
    S0 = O.cycle_d(ii, jj, rij.reshape(-1, 9), st)
    res = O.pgd_run(st, S0, iters, **step)
    return st, S0, res


def c_params(iters, step_kind=0, lr=0.01, beta1=0.9, beta2=0.999, decay_interval=25, hybrid_strategy=0,
             t0=0, patience=30, stop_tol=1e-5, seed=0, check_every=0):
    p = _lib.default_params()
    p.iters = iters; p.step_kind = step_kind; p.lr = lr; p.beta1 = beta1; p.beta2 = beta2
    p.decay_interval = decay_interval; p.hybrid_strategy = hybrid_strategy; p.t0 = t0
    p.patience = patience; p.stop_tol = stop_tol; p.seed = seed; p.check_every = check_every
    return p


STRUCT_KEYS = ("pos_edge", "cum_ind", "k", "e_jk", "e_ki", "ikj", "jki")


def assert_structure_equal(a, b):
    assert a["m_pos"] == b["m_pos"] and a["m_cycle"] == b["m_cycle"] and a["n_sample"] == b["n_sample"]
    for key in STRUCT_KEYS:
        assert np.array_equal(a[key], b[key]), key


def csr(nn, ii, jj):
    """CSR adjacency (neighbours ascending) with the edge id of every slot, as the library builds it: (rowptr, adj, adj_eid, row_of)."""
    m = ii.shape[0]
    src = np.concatenate([ii, jj]); dst = np.concatenate([jj, ii]); eid = np.concatenate([np.arange(m), np.arange(m)])
    order = np.lexsort((dst, src))
    rowptr = np.zeros(nn + 1, dtype=np.int64)
    np.add.at(rowptr, src + 1, 1)
    return np.cumsum(rowptr), dst[order], eid[order], src[order]


def reduce_scatter_by_hand(shards):
    """The reduce-scatter of the mirror sums between emulated ranks, part by part (desc_shard_info.xparts): blocks [c * world, (c + 1) * world)
    of every rank's T, added -> block c of every rank's T_recv."""
    import torch
    world = len(shards)
    Lp, X = shards[0].info.t_part, shards[0].info.xparts
    for c in range(X):
        tot = torch.zeros(world * Lp, dtype=shards[0].T.dtype, device=shards[0].T.device)
        for s in shards:
            tot += s.T[c * world * Lp:(c + 1) * world * Lp]
        for r, s in enumerate(shards):
            s.T_recv[c * Lp:(c + 1) * Lp].copy_(tot.view(world, Lp)[r])


def emulate_sharded(lib, nn, ii, jj, rij, p, world, check_every=5, where=None, nmin=30, probe=None):
    """`world` ranks emulated in one process on one GPU: every rank's shard on the same card and stream, the collectives done by hand
    between their exchange buffers.  Returns every rank's download (with the sweep it launched last) and its (seg_lo, seg_hi, cyc_lo, cyc_hi).
    probe(shards), if given, is called after the iteration loop and before the final objective exchange, inside the ranks' stream context:
    the shards then hold the weights of the last sweep (tests/test_gpu_colsum.py reads the column sums there)."""
    import torch
    from desc_amd.sharded import HipShard
    prob = lib.ProblemArrays(nn, ii, jj, rij)
    st = lib.Structure.build(prob, nmin, p.seed, lib.BUILD_HOST if where is None else where, 0)
    stream = torch.cuda.Stream(torch.device("cuda", 0))      # one stream for every emulated rank
    shards = [HipShard(prob, st, 0, r, world, stream=stream) for r in range(world)]
    st.free()
    L = shards[0].slice_len
    ctx = torch.cuda.stream(stream)
    ctx.__enter__()

    def all_gather():
        for r in range(world):
            piece = shards[r].sall.view(world, L)[r].clone()
            for s in shards:
                s.sall.view(world, L)[r].copy_(piece)

    for s in shards: s.reset(p)
    for s in shards: s.finish(1)
    all_gather()
    for s in shards: s.finish(2)
    left = p.iters
    while left > 0:
        n = min(left, check_every)
        for _ in range(n):
            for s in shards: s.colsum()
            reduce_scatter_by_hand(shards)
            for s in shards: s.sweep()
            all_gather()
            for s in shards: s.finish(0)
        left -= n
        flags = [s.stopped() for s in shards]
        assert len(set(flags)) == 1
        if left > 0 and flags[0]:
            break
    if probe is not None:
        try:
            probe(shards)
        except BaseException:                                # a failing probe leaves neither the stream context nor the shards behind
            ctx.__exit__(None, None, None)
            for s in shards: s.destroy()
            raise
    for s in shards: s.objective(0)
    all_gather()
    for s in shards: s.objective(1)
    outs = [s.download() for s in shards]
    ctx.__exit__(None, None, None)
    segs = [(s.info.seg_lo, s.info.seg_hi, s.info.cyc_lo, s.info.cyc_hi) for s in shards]
    for o, s in zip(outs, shards):
        o["last_sweep"], o["kernel"] = s.solver.last_sweep(), s.solver.kernel_name()
    for s in shards: s.destroy()
    return outs, segs


def run_unsharded(lib, prob, st, p):
    """One rank through the plain path on a structure built by the caller (its n_sample_min and seed are the caller's)."""
    solver = lib.Solver(prob, st, 0)
    out = solver.run(p)
    out["kernel"], out["last_sweep"] = solver.kernel_name(), solver.last_sweep()
    solver.destroy()
    return out

"""TEST INFRASTRUCTURE -- the problems of the tests that run every batched call at the largest size its create call accepts
(tests/test_batch_caps_host.py, tests/test_gpu_batch_caps.py), built once per process.  Every size is read from the library
(refine_batch_max_n() and the like); the figures below are what the present caps give, and tests/test_batch_caps_host.py asserts them.

All graphs are sparse, so that one workgroup finishes in milliseconds and the CPU restatements in seconds.

laa_cap()     Uniform_Topology(748, 12/747, 0.2, 0.1, seed=109): m = 4496, connected.  With S = noisy_S(mo, 361) and the plain spectral
              start desc_refine_oracle takes 19 iterations (final score 9.77e-4), and the same 19 with the threshold moved by +-0.1 %.
              With the demo's MPLS parameters, nsample = 20 and sampling seed MPLS_SEED, mpls_oracle takes 26 iterations on its own
              tree (final score 9.50e-4), and no step's score lies within 0.1 % of stop_threshold.
              Seed 61 (m = 4497, 26 iterations, final score 9.56e-4) was passed over: the spectral start of its node 349 is a turn of
              pi - 1.3e-3, where Utils/R2Q.m divides by q0 = 6.5e-4 and returns a quaternion whose norm is off 1 by 1.6e-10; the
              reference keeps unnormalised quaternions, so the oracle's own result there is 3.2e-12 off a rotation, and the device's
              2.7e-12 (the same bits from the single call): above the 1e-12 the results are held to, with nothing wrong in a kernel.
              Among seeds 61 and 77 .. 109, 109 has the start farthest from such a turn (smallest q0 4.4e-3); its oracle result is
              2.6e-13 off a rotation.
laa_cap_minus_one(), laa_n513()   n = cap - 1 and n = 513 (the first row of the third block of 256 rows), the same density.  Their
              start is the ground truth turned by 0.05 rad per node (refine_batch_cases.dense_case): compared with the single call only.
irls_cap()    Uniform_Topology(557, 12/556, 0.2, 0.1, seed=67): m = 3420, connected; tests/irls_oracle.py takes 10 L1 and 23 reweighted
              iterations and 60 primal-dual steps, and under one ulp of RijMat (graph_shapes.ulp_perturbed) its R_l1 moves by 3.4e-12
              and its R by 9.8e-12, within 1/100 of the 1e-9 and 1e-7 the device is held to (the rule of tests/test_graph_shapes.py).
              Seeds 62 (m = 3266) and 66 were passed over: there R_l1 moves by 1.4e-9 and 2.6e-10 under one ulp, and the device was
              2.7e-9 from the oracle on seed 62.  irls_n513(): 513 nodes, compared with the single call only.
mst_cap()     4096 nodes: the path under the four weight kinds of tests/test_graph_shapes.py, the star with its hub at node 1 and at
              node 4096 under the same four, and ER(0.0015) plus a Hamiltonian path with noisy_truth weights.
row_cap(hub)  graph_shapes.hub(4097, 0.002, [hub], q=0.0, sigma=0.2, seed=72): the hub's row has 4096 entries, exactly what the sampler
              stages; hub = 2000 (m = 24 991, the next longest row 24, the shortest 4), 1 and 4097 (the long row as row i and as row j
              of every pair it is in).  Noise but no outliers, as every shape CEMP's SVec is compared on (tests/graph_shapes.py:
              SHAPES): with q = 0.2 cemp_oracle_batched moves by 5.5e-13 under one ulp of RijMat (a Haar outlier cycle within 1e-4 of
              pi, where acos turns 1 ulp of the trace into 1e-12 of S0) and the device was 3.1e-12 from it with the hub at node 4097;
              with q = 0 the oracle moves by at most 1.6e-14.  The pattern of the graph, which is what the staging depends on, is
              the same for every q.
pgd_dense()   Uniform_Topology(90, 0.9, 0.2, 0.1, seed=71): m = 3599, codegrees 60 .. 82 with median 71, so ceil(median / 4) = 18 and
              n_sample = max(18, n_sample_min): T for the T >= 18 of PGD_T, and then every segment is exactly T cycles long up to
              T = 33; 98.4 % of the edges have a codegree >= 64, so at T = 64 3542 segments fill a 64-lane group.
pgd_mid()     Uniform_Topology(90, 0.8, 0.2, 0.1, seed=71): m = 3212, codegrees 41 .. 71 with median 57, so ceil(median / 4) = 15:
              at T = 16 and 17, where pgd_dense() stays at n_sample = 18, n_sample = T here and all 3212 segments are exactly T long
              (a full 16-lane group, and the first segment past one).  No graph has both a median codegree of at most 64 (n_sample
              = 16 at T = 16) and, at 90 nodes, 3000 edges of codegree >= 64, so the two ride in the same batch.
pgd_sparse()  the 12-node problem of tests/test_gpu_batch.py (longest segment 5): a 16-lane group that is not full, in the same launch."""
import numpy as np

from desc_amd.models import Uniform_Topology
from tests import graph_shapes as gs
from tests import refine_batch_cases
from tests.irls_batch_cases import connected          # noqa: F401  (used by tests/test_batch_caps_host.py as cases.connected)

_cache = {}
PGD_T = (16, 17, 31, 32, 33, 63, 64)
PGD_DENSE_MIN_T = 18           # ceil(median codegree / 4) of pgd_dense(): below it pgd_mid() is the problem whose n_sample is T
PGD_SEED = 1
LAA_SEED = 109
LAA_SMALL = 3
IRLS_SEED = 67
REFINE_ITERS = 19              # final score 9.77e-4
MPLS_SEED = 161
MPLS_ITERS = 26                # on the oracle's own tree; final score 9.50e-4
MST_KINDS = ("increasing", "decreasing", "alternating", "equal")


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def caps():
    """The caps the library reports."""
    from desc_amd import _lib
    return dict(refine=_lib.refine_batch_max_n(), mpls=_lib.mpls_batch_max_n(), irls=_lib.irls_batch_max_n(), mst=_lib.mst_batch_max_n(),
                row=_lib.cemp_batch_max_degree())


def _sparse(n, seed):
    return Uniform_Topology(n, 12.0 / (n - 1), 0.2, 0.1, "uniform", seed=seed)


# ---- the Lie-algebraic averaging core: refinement and MPLS ---------------------------------------------------------------------
def laa_cap():
    return _once("laa_cap", lambda: _sparse(caps()["refine"], LAA_SEED))


def laa_cap_minus_one():
    return _once("laa_cap-1", lambda: _sparse(caps()["refine"] - 1, 64))


def laa_n513():
    return _once("laa_513", lambda: _sparse(513, 63))


def laa_small():
    """Entry LAA_SMALL of refine_batch_cases.models() (n = 90) with its inputs: (model, S, R_init).  (Entry 2, n = 40, has a start like
    seed 61's above: the oracle's own result is 2.5e-12 off a rotation, the device's 2.0e-12.)"""
    S, R0 = refine_batch_cases.inputs()
    return refine_batch_cases.models()[LAA_SMALL], S[LAA_SMALL], R0[LAA_SMALL]


def laa_cap_inputs():
    """(S, R_init) of laa_cap(): noisy_S(mo, 361) and the plain spectral solution (a dense eigen-solve of 2244 rows, once)."""
    def make():
        from oracle.spectral_oracle import spectral_oracle
        mo = laa_cap()
        return refine_batch_cases.noisy_S(mo, 361), spectral_oracle(mo.Ind, mo.RijMat)
    return _once("laa_cap_inputs", make)


def turned_truth_inputs(mo, seed):
    """(S, R_init) as refine_batch_cases.dense_case(): S = noisy_S, R_init = the ground truth turned by 0.05 rad about a random axis."""
    def make():
        n = int(mo.Ind.max())
        ax = np.random.default_rng(seed).standard_normal((n, 3))
        ax *= 0.05 / np.linalg.norm(ax, axis=1)[:, None]
        Rg = np.transpose(np.asarray(mo.R_orig), (2, 0, 1))
        return refine_batch_cases.noisy_S(mo, seed), np.asfortranarray(np.transpose(Rg @ refine_batch_cases._rotvec(ax), (1, 2, 0)))
    return _once(("turned", id(mo), seed), make)


def refine_oracle_result(stop_threshold=1e-3):
    """desc_refine_oracle on laa_cap(): (R_ref, iters_ref, score_ref), once per threshold."""
    def make():
        from oracle.refine_oracle import desc_refine_oracle
        mo = laa_cap()
        S, R0 = laa_cap_inputs()
        return desc_refine_oracle(mo.Ind, mo.RijMat, S, R0, stop_threshold=stop_threshold)
    return _once(("refine_oracle", stop_threshold), make)


def mpls_oracle_result(svec_for_tree=None, stop_threshold=1e-3):
    """mpls_oracle on laa_cap() with the demo's parameters and MPLS_SEED, the tree built from ``svec_for_tree`` (the device's SVec;
    None: the oracle's own).  Once per (threshold, whether an SVec was given)."""
    def make():
        from tests.mpls_batch_cases import demo_params
        from tests.mpls_oracle import mpls_oracle
        mo = laa_cap()
        cemp, mpls = demo_params(stop_threshold=stop_threshold)
        return mpls_oracle(mo.Ind, mo.RijMat, cemp, mpls, seed=MPLS_SEED, svec_for_tree=svec_for_tree)
    return _once(("mpls_oracle", stop_threshold, svec_for_tree is not None), make)


def stop_is_clear(scores, stop_threshold, margin=1e-3):
    """The loop 'while score > stop_threshold' that produced ``scores`` stops at the same step for every threshold within ``margin``
    (relative) of stop_threshold: every score but the last lies above that band and the last one below it."""
    lo, hi = stop_threshold * (1 - margin), stop_threshold * (1 + margin)
    return all(x > hi for x in scores[:-1]) and scores[-1] < lo


# ---- IRLS ------------------------------------------------------------------------------------------------------------------------
def irls_cap():
    def make():
        mo = _sparse(caps()["irls"], IRLS_SEED)
        return mo.Ind, mo.RijMat
    return _once("irls_cap", make)


def irls_n513():
    def make():
        mo = _sparse(513, 65)
        return mo.Ind, mo.RijMat
    return _once("irls_513", make)


# ---- the tree kernel -------------------------------------------------------------------------------------------------------------
def mst_weights(kind, m):
    """tests/test_graph_shapes.py: mst_weights."""
    e = np.arange(m)
    return {"increasing": e / m, "decreasing": 1.0 - e / m, "alternating": 0.5 * (e % 2), "equal": np.full(m, 0.25)}[kind]


def mst_cap():
    """A list of (name, model, S): 4 paths, 8 stars, 1 random graph, all of mst_batch_max_n() nodes."""
    def make():
        n = caps()["mst"]
        out = []
        path = gs.band(n, 1, seed=3)
        out += [("path-" + kind, path, mst_weights(kind, n - 1)) for kind in MST_KINDS]
        for hub_id in (1, n):
            star = gs.star(n, hub_id, seed=4)
            out += [("star%d-%s" % (hub_id, kind), star, mst_weights(kind, n - 1)) for kind in MST_KINDS]
        er = gs.hub(n, 0.0015, [], seed=73)
        out.append(("er", er, gs.noisy_truth(er, 5)))
        return out
    return _once("mst_cap", make)


# ---- the sampler's staged row ----------------------------------------------------------------------------------------------------
def row_cap(hub_id=2000):
    """hub(cap + 1, 0.002, [hub_id], q=0.0, sigma=0.2, seed=72); hub_id = -1 stands for the last node."""
    cap = caps()["row"]
    hub_id = cap + 1 if hub_id == -1 else hub_id
    return _once(("row_cap", hub_id), lambda: gs.hub(cap + 1, 0.002, [hub_id], q=0.0, sigma=0.2, seed=72))


def hub_edges(mo, hub_id):
    """Rows of Ind with the hub at either end."""
    return np.flatnonzero((mo.Ind[:, 0] == hub_id) | (mo.Ind[:, 1] == hub_id))


def sampled_edges_oracle(Ind, rows, nsample, seed):
    """The keyed sampling rule of tests/mpls_oracle.py: cemp_stage (:38-47) for the edges ``rows`` alone, without the n x n tables:
    (e_jk, e_ki), each len(rows) x nsample edge ids; -1 in the rows of an edge without a common neighbour."""
    from oracle.cemp_oracle import _mix64_v
    Ind = np.asarray(Ind, dtype=np.int64)
    n, m = int(Ind.max()), Ind.shape[0]
    order = np.argsort(np.concatenate([Ind[:, 0], Ind[:, 1]]), kind="stable")
    nbr = np.concatenate([Ind[:, 1], Ind[:, 0]])[order]
    nbr_e = np.concatenate([np.arange(m), np.arange(m)])[order]
    ptr = np.searchsorted(np.concatenate([Ind[:, 0], Ind[:, 1]])[order], np.arange(1, n + 2))
    e_jk = np.full((len(rows), nsample), -1, dtype=np.int64); e_ki = e_jk.copy()
    tt = np.arange(nsample, dtype=np.uint64)
    for r, e in enumerate(rows):
        i, j = int(Ind[e, 0]), int(Ind[e, 1])
        ni, nj = nbr[ptr[i - 1]:ptr[i]], nbr[ptr[j - 1]:ptr[j]]
        common, at_i, at_j = np.intersect1d(ni, nj, return_indices=True)               # ascending node ids, as flatnonzero(common[e])
        if common.size == 0:
            continue
        with np.errstate(over="ignore"):
            key = _mix64_v(_mix64_v(np.uint64(seed) ^ ((np.uint64(e) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)))
                           ^ ((tt + np.uint64(1)) * np.uint64(0xD1B54A32D192ED03)))
        idx = (key % np.uint64(common.size)).astype(np.int64)
        e_ki[r] = nbr_e[ptr[i - 1]:ptr[i]][at_i][idx]
        e_jk[r] = nbr_e[ptr[j - 1]:ptr[j]][at_j][idx]
    return e_jk, e_ki


# ---- the batched PGD ---------------------------------------------------------------------------------------------------------------
def _pgd(n, p, seed):
    from tests.helpers import make_problem
    mo, nn, ii, jj, rij = make_problem("uniform", n=n, p=p, q=0.2, sigma=0.1, seed=seed)
    return dict(mo=mo, n=nn, ii=ii, jj=jj, rij=rij)


def pgd_dense():
    return _once("pgd_dense", lambda: _pgd(90, 0.9, 71))


def pgd_mid():
    return _once("pgd_mid", lambda: _pgd(90, 0.8, 71))


def pgd_sparse():
    return _once("pgd_sparse", lambda: _pgd(12, 0.6, 9))


def pgd_reference(O, which, T, iters=40, **step):
    """(structure, S0, pgd_run result) of the oracle ``O`` (the ``oracle`` fixture) on pgd_dense() / pgd_sparse() with n_sample_min = T;
    the structure and S0 once per (problem, T), a run once per parameter set.  ``step`` may hold adam=True: the run gets zeroed moment
    vectors, returned as a fourth and fifth entry."""
    q = {"dense": pgd_dense, "mid": pgd_mid, "sparse": pgd_sparse}[which]()

    def structure():
        st = O.build_structure(q["n"], q["ii"], q["jj"], seed=PGD_SEED, n_sample_min=T)
        return st, O.cycle_d(q["ii"], q["jj"], q["rij"].reshape(-1, 9), st)
    st, S0 = _once(("pgd_st", which, T), structure)

    def run():
        kw = dict(step)
        if kw.pop("adam", False):
            am, av = np.zeros(st["m_cycle"]), np.zeros(st["m_cycle"])
            return O.pgd_run(st, S0, iters, adam_m=am, adam_v=av, **kw), am, av
        return O.pgd_run(st, S0, iters, **kw), None, None
    ref, am, av = _once(("pgd_run", which, T, iters, tuple(sorted(step.items()))), run)
    return st, S0, ref, am, av

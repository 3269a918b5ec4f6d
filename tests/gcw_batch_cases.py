"""TEST INFRASTRUCTURE -- the problems of the batched eigen-solve's tests (tests/test_gcw_batch_host.py, tests/test_gpu_gcw_batch.py),
built once per process.

The mixed batch: the smallest sizes at which the kernel can go wrong -- fewer item rounds than threads (n = 8, 12, band(10, 2)), several
rounds (40, 90, 150) and exactly the cap.  Oracle gaps lambda_3 - lambda_4 of these problems, computed on the CPU with the seeds below
(GCW operator with S = noisy_truth / Spectral operator): 0.26 / 0.89, 0.045 / 1.7, 0.19 / 10.6, 0.28 / 24.4, 0.32 / 24.7, 0.14 / 11.6,
band 0.053 / 0.55 -- the dense oracle's top eigenvectors are well defined for all of them."""
import numpy as np

from desc_amd.models import Uniform_Topology
from tests import graph_shapes as gs

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def mixed_models(max_n):
    """(n, p) = (8, .9), (12, .6), (40, .5), (90, .5), (150, .3), (max_n, mean degree ~ 25) and band(10, 2); q = 0.2, sigma = 0.1."""
    def make():
        mos = [Uniform_Topology(n, p, 0.2, 0.1, "uniform", seed=s) for n, p, s in
               ((8, 0.9, 31), (12, 0.6, 32), (40, 0.5, 33), (90, 0.5, 34), (150, 0.3, 35), (max_n, 25.0 / (max_n - 1), 36))]
        mos.append(gs.band(10, 2, seed=37))
        assert [int(mo.Ind.max()) for mo in mos] == [8, 12, 40, 90, 150, max_n, 10]
        return mos
    return _once(("mixed", max_n), make)


def mixed_S(max_n):
    return _once(("mixed_S", max_n), lambda: [gs.noisy_truth(mo, 100 + k) for k, mo in enumerate(mixed_models(max_n))])


def single_edge(seed=39):
    """n = 2: rows == block width, spectrum +-1 three times each."""
    return _once(("edge", seed), lambda: gs._measure(2, [(1, 2)], 0.0, 0.1, np.random.default_rng(seed)))


def many_small(count=300):
    """Uniform_Topology(12, 0.6, 0.2, 0.1) with seeds 1000 .. and S = noisy_truth with seeds 2000 ..: on the CPU every one of the 300 has
    an oracle gap above 1e-3 (none is left out)."""
    def make():
        mos = [Uniform_Topology(12, 0.6, 0.2, 0.1, "uniform", seed=1000 + s) for s in range(count)]
        return mos, [gs.noisy_truth(mo, 2000 + s) for s, mo in enumerate(mos)]
    return _once(("many", count), make)


def gcw_gap(mo, S):
    """lambda_3 - lambda_4 of the symmetrised GCW operator D^-1/2 (W o R) D^-1/2 (dense)."""
    from oracle.spectral_oracle import _blk
    Ind = np.asarray(mo.Ind); n = int(Ind.max())
    W = np.zeros((n, n)); W[Ind[:, 0] - 1, Ind[:, 1] - 1] = 1.0 / (np.asarray(S) ** 1.5 + 1e-8); W = W + W.T
    d = W.sum(axis=1)
    di = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    lam = np.linalg.eigvalsh(_blk(Ind, mo.RijMat, n) * np.kron(di[:, None] * W * di[None, :], np.ones((3, 3))))
    return float(lam[-3] - lam[-4])


def with_empty_row(seed=41, hole=10):
    """A 20-node problem in which node ``hole`` (1-based, interior) occurs in no edge; the other 19 nodes stay connected."""
    def make():
        mo = Uniform_Topology(20, 0.5, 0.2, 0.1, "uniform", seed=seed)
        keep = (mo.Ind[:, 0] != hole) & (mo.Ind[:, 1] != hole)
        Ind, Rij = mo.Ind[keep], np.asfortranarray(mo.RijMat[:, :, keep])
        assert int(Ind.max()) == 20 and hole not in Ind
        others = np.array([v for v in range(1, 21) if v != hole])
        lv = gs.bfs_levels(Ind, root=1)
        assert (lv[others - 1] >= 0).all()
        return Ind, Rij, gs.noisy_truth(mo, 7)[keep]
    return _once(("hole", seed, hole), make)


def csr_numpy(n, ii, jj):
    """CSR of the undirected graph, neighbours ascending, edge id per slot (0-based endpoints sorted by (i, j))."""
    m = ii.shape[0]
    src = np.concatenate([ii, jj]); dst = np.concatenate([jj, ii]); eid = np.concatenate([np.arange(m), np.arange(m)])
    order = np.lexsort((dst, src))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))])
    return rowptr.astype(np.int32), dst[order].astype(np.int32), eid[order].astype(np.int32)

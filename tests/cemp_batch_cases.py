"""TEST INFRASTRUCTURE -- the problems of the batched CEMP / tree tests (tests/test_cemp_batch_host.py, tests/test_gpu_cemp_batch.py),
built once per process, and the oracle's answers, computed once and shared.

The twelve graphs (BETA = 2 ** arange(6), max_iter = 6, nsample = 50, seed = 1; checked on the CPU with cemp_oracle_batched / kruskal):
all connected, all touching every node id.  U8 .. U150: every edge on a cycle.  band10_2: codegrees <= 2.  bridged: exactly the 2 bridges
have no cycle (CEMP-GCW gap lambda_3 - lambda_4 only 0.002: not in the eigen-solve comparison; >= 0.23 for the eleven others).  star12:
no cycle at all, every tree key equal.  pend30: 4 edges without a cycle.  U100d: every codegree between 65 and 91, rows of up to 96.
hub300: one row of 299.  U278: 345 edges without a cycle, 433 duplicate S + 1 keys."""
import numpy as np

from desc_amd.models import Uniform_Topology
from oracle.cemp_oracle import cemp_oracle, cemp_oracle_batched
from tests import graph_shapes as gs

BETA = [2.0 ** k for k in range(6)]
NAMES = ["U8", "U12", "U40", "U90", "U150", "band10_2", "bridged", "star12", "pend30", "U100d", "hub300", "U278"]
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def params(nsample=50, seed=1, max_iter=6, reweighting=None):
    return dict(max_iter=max_iter, reweighting=BETA if reweighting is None else reweighting, nsample=nsample, seed=seed)


def _make(name):
    U = {"U8": (8, 0.9, 31), "U12": (12, 0.6, 32), "U40": (40, 0.5, 33), "U90": (90, 0.5, 34), "U150": (150, 0.3, 35), "U100d": (100, 0.9, 44),
         "U278": (278, 25.0 / 277, 36)}
    if name in U:
        n, p, s = U[name]
        return Uniform_Topology(n, p, 0.2, 0.1, "uniform", seed=s)
    return {"band10_2": lambda: gs.band(10, 2, seed=37), "bridged": lambda: gs.bridged(20, 15, 0.5, 0.5, 2, seed=41),
            "star12": lambda: gs.star(12, 3, seed=38), "pend30": lambda: gs.dense_with_pendants(30, 0.5, 4, seed=42),
            "hub300": lambda: gs.hub(300, 0.02, [150], seed=43)}[name]()


def model(name):
    return _once(("model", name), lambda: _make(name))


def models(names):
    return [model(k) for k in names]


def no_cycle(name):
    """Edges of the graph that lie on no 3-cycle (bool per row of Ind)."""
    return _once(("nocycle", name), lambda: gs.codegrees(model(name).Ind) == 0)


def oracle_S(name, nsample=50, seed=1, max_iter=6, reweighting=None, literal=False):
    """cemp_oracle_batched (or the literal cemp_oracle) on one of the twelve graphs: computed once per parameter set."""
    beta = BETA if reweighting is None else list(reweighting)
    mo = model(name)
    fn = cemp_oracle if literal else cemp_oracle_batched
    return _once(("S", name, nsample, seed, max_iter, tuple(beta), literal), lambda: fn(mo.Ind, mo.RijMat, max_iter, beta, nsample, seed))


def permuted(name, seed=1):
    """(Ind as Fortran-ordered doubles with its rows permuted, RijMat permuted alike, perm): row t of the result is row perm[t] of the model."""
    def make():
        mo = model(name)
        perm = np.random.default_rng(seed).permutation(mo.Ind.shape[0])
        return np.asfortranarray(mo.Ind[perm].astype(np.float64)), np.asfortranarray(mo.RijMat[:, :, perm]), perm
    return _once(("perm", name, seed), make)


def many_small(count=300):
    return _once(("many", count), lambda: [Uniform_Topology(12, 0.6, 0.2, 0.1, "uniform", seed=1000 + s) for s in range(count)])


def two_triangles():
    """The disconnected problem of tests/test_gpu_mpls.py."""
    def make():
        rng = np.random.default_rng(4)
        Q = np.linalg.qr(rng.standard_normal((6, 3, 3)))[0]
        Q[np.linalg.det(Q) < 0, :, 0] *= -1
        return np.array([[1, 2], [1, 3], [2, 3], [4, 5], [4, 6], [5, 6]]), np.ascontiguousarray(np.transpose(Q, (1, 2, 0)))
    return _once("triangles", make)

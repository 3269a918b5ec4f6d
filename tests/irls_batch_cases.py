"""TEST INFRASTRUCTURE -- the problems of the batched IRLS tests (tests/test_irls_batch_host.py, tests/test_gpu_irls_batch.py), built
once per process.

All are Uniform_Topology(n, p, q, sigma, "uniform", seed), chosen as the smallest shapes at which the workgroup can go wrong: m below
one virtual block of the partial-reduction kernels (256 edges) and exactly at its edge, more than one virtual block, n across 256
(the second pass of the dot products and score chunks, the node terms of virtual block 1), and the early-stop branch of the L1 loop.
tests/irls_oracle.py gives on the six TABLE problems (CPU): all connected, pd_ill = pd_stuck = warned = 0, pd_steps 60 everywhere
except the first (48), and the iteration counts of TABLE below at MaxIterations = (10, 100)."""
import numpy as np

from desc_amd.models import Uniform_Topology

_cache = {}

# (n, p, q, sigma, seed), m, l1_iters, irls_iters GM, irls_iters L12, pd_steps
TABLE = (
    ((16, 0.5, 0.1, 0.05, 1), 58, 8, 8, 10, 48),        # the L1Step x 4 branch
    ((23, 0.7, 0.2, 0.1, 2), 183, 10, 18, 20, 60),
    ((40, 0.5, 0.3, 0.1, 3), 395, 10, 20, 16, 60),
    ((100, 0.5, 0.2, 0.1, 4), 2483, 10, 13, 15, 60),
    ((100, 0.3, 0.4, 0.1, 5), 1532, 10, 19, 18, 60),
    ((257, 0.12, 0.2, 0.1, 6), 3946, 10, 19, 12, 60),
)
ORACLE_CASE = 6      # index in problems(): Uniform_Topology(30, 0.5, 0.1, 0.05, seed=1), held to 1e-9 in R_l1 by tests/test_gpu_irls.py


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def connected(Ind):
    """Every node id in 1..max(Ind) is reached from node 1 (a plain union-find over the rows)."""
    Ind = np.asarray(Ind, dtype=np.int64)
    n = int(Ind.max())
    parent = list(range(n + 1))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for i, j in Ind:
        parent[find(int(i))] = find(int(j))
    return len({find(v) for v in range(1, n + 1)}) == 1


def cut(Ind, RijMat, m):
    """The first rows of (Ind, RijMat) cut down to exactly m: rows are dropped from the end while the graph stays connected (a row whose
    removal would disconnect it is kept)."""
    Ind, keep = np.asarray(Ind), list(range(Ind.shape[0]))
    t = len(keep) - 1
    while len(keep) > m and t >= 0:
        trial = keep[:t] + keep[t + 1:]
        if connected(Ind[trial]) and int(Ind[trial].max()) == int(Ind.max()):
            keep = trial
        t -= 1
    assert len(keep) == m and connected(Ind[keep])
    return Ind[keep], RijMat[:, :, keep]


def triangle():
    """A noisy triangle: n = 3, m = 3."""
    rng = np.random.default_rng(11)
    Ind = np.array([[1, 2], [1, 3], [2, 3]])
    Q = np.linalg.qr(rng.standard_normal((3, 3, 3)))[0]
    Q[np.linalg.det(Q) < 0, :, 0] *= -1
    Rij = np.empty((3, 3, 3))
    for k, (i, j) in enumerate(Ind - 1):
        N = np.linalg.qr(np.eye(3) + 0.05 * rng.standard_normal((3, 3)))[0]
        N = N if np.linalg.det(N) > 0 else -N
        Rij[:, :, k] = Q[i] @ Q[j].T @ N
    return Ind, Rij


def problems():
    """The ten (Ind, RijMat) pairs: TABLE's six, the 30-node oracle problem, the triangle, the 40-node problem cut to 256 and to 257
    edges."""
    def make():
        out = []
        for (args, m, *_rest) in TABLE:
            mo = Uniform_Topology(*args[:4], "uniform", seed=args[4])
            assert mo.Ind.shape[0] == m and connected(mo.Ind)
            out.append((mo.Ind, mo.RijMat))
        mo = Uniform_Topology(30, 0.5, 0.1, 0.05, "uniform", seed=1)
        out.append((mo.Ind, mo.RijMat))
        out.append(triangle())
        Ind40, R40 = out[2]
        out.append(cut(Ind40, R40, 256))
        out.append(cut(Ind40, R40, 257))
        for Ind, _ in out:
            assert connected(Ind)
        return out
    return _once("problems", make)


def shuffled(k, seed=0):
    """Problem k with its Ind rows shuffled: the caller's row order -- and with it the spanning-tree start -- differs from the sorted
    one.  (A pair given as (j, i) is refused by the library's input rule Ind(:,1) < Ind(:,2), by the single call and by the batch alike:
    flipped() below is such a problem, for the refusal tests.)"""
    def make():
        Ind, Rij = problems()[k]
        perm = np.random.default_rng(1000 + seed + k).permutation(Ind.shape[0])
        return Ind[perm].copy(), Rij[:, :, perm].copy()
    return _once(("shuffled", k, seed), make)


def flipped(k):
    """shuffled(k) with every third pair given as (j, i) and the transposed block."""
    Ind, Rij = shuffled(k)
    Ind, Rij = Ind.copy(), Rij.copy()
    flip = np.arange(Ind.shape[0]) % 3 == 0
    Ind[flip] = Ind[flip][:, ::-1]
    Rij[:, :, flip] = np.transpose(Rij[:, :, flip], (1, 0, 2))
    return Ind, Rij


def planar():
    """The 16-node graph with noisy rotations about the z axis alone: the x and y coordinates of every edge's log map are exactly zero,
    the degenerate right-hand side on which l1decode_pd returns early."""
    def make():
        Ind, _ = problems()[0]
        rng = np.random.default_rng(21)
        th = rng.uniform(-np.pi, np.pi, int(Ind.max()))
        ang = th[Ind[:, 0] - 1] - th[Ind[:, 1] - 1] + 0.05 * rng.standard_normal(Ind.shape[0])
        Rij = np.zeros((3, 3, Ind.shape[0]))
        Rij[0, 0], Rij[0, 1], Rij[1, 0], Rij[1, 1], Rij[2, 2] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang), 1.0
        return Ind, Rij
    return _once("planar", make)


def path_graph(n=9):
    """A path 1 - 2 - ... - n whose rows are listed from the far end: every pass of the tree start reaches one more node."""
    rng = np.random.default_rng(5)
    Ind = np.array([[v, v + 1] for v in range(n - 1, 0, -1)])
    Q = np.linalg.qr(rng.standard_normal((n - 1, 3, 3)))[0]
    Q[np.linalg.det(Q) < 0, :, 0] *= -1
    return Ind, np.ascontiguousarray(np.transpose(Q, (1, 2, 0)))


def single(mode, k_or_pair, MaxIterations=(10, 100), SIGMA=5):
    """IRLS_GM / IRLS_L12 with return_info on problem k (or on an (Ind, RijMat) pair, not cached): computed once per process and left
    unchanged."""
    from desc_amd import IRLS_GM, IRLS_L12
    fn = {"GM": IRLS_GM, "L12": IRLS_L12}[mode]
    if not isinstance(k_or_pair, int):
        Ind, Rij = k_or_pair
        return fn(Rij, Ind, SIGMA=SIGMA, MaxIterations=MaxIterations, return_info=True)
    Ind, Rij = problems()[k_or_pair]
    return _once(("single", mode, k_or_pair, tuple(MaxIterations), SIGMA),
                 lambda: fn(Rij, Ind, SIGMA=SIGMA, MaxIterations=MaxIterations, return_info=True))

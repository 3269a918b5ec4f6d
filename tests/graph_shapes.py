"""TEST INFRASTRUCTURE -- seeded graph families whose *shape* is not Erdos-Renyi: hubs, bands, stars, bipartite, bridged, power-law,
dense with pendants, two components, books.  Every family builds an adjacency pattern and then applies the measurement model of
``Uniform_Topology`` (desc_amd/models.py:88-104): Haar ground truth, noise of size ``sigma`` on the good edges, Haar outliers with
probability ``q``.  The struct returned is the one ``Uniform_Topology`` returns: ``Ind`` (m x 2, 1-based, i < j, sorted by (i, j)),
``RijMat``, ``Rij_orig``, ``R_orig``, ``ErrVec``, ``corrupted``, ``AdjMat``.

Every family except ``two_components`` is connected and touches every node id in 1..n (tests/test_graph_shapes.py checks it).
Node ids are 1-based throughout, as in ``Ind``."""
import numpy as np

from desc_amd.models import _finish, _haar, _project_so3


def _measure(n, pairs, q, sigma, rng):
    """pairs: iterable of 1-based (i, j), any order, duplicates allowed -> the model struct."""
    P = np.asarray(list(pairs) if not isinstance(pairs, np.ndarray) else pairs, dtype=np.int64).reshape(-1, 2)
    P = np.unique(np.sort(P[P[:, 0] != P[:, 1]], axis=1), axis=0)             # i < j, sorted by (i, j)
    Ind_i, Ind_j = P[:, 0], P[:, 1]
    m = P.shape[0]
    R_orig = _haar(rng, n)
    Rij_orig = R_orig[Ind_i - 1] @ np.transpose(R_orig[Ind_j - 1], (0, 2, 1))
    Rm = Rij_orig.copy()
    good = rng.random(m) >= q
    gi, ci = np.flatnonzero(good), np.flatnonzero(~good)
    if gi.size:
        Rm[gi] = _project_so3(Rm[gi] + sigma * rng.standard_normal((gi.size, 3, 3)))
    if ci.size:
        Rm[ci] = _haar(rng, ci.size)
    return _finish(n, Ind_i, Ind_j, Rm, Rij_orig, R_orig, dict(corrupted=~good))


def _er_pairs(rng, nodes, p):
    """Erdos-Renyi on the given (1-based) node ids."""
    nodes = np.asarray(nodes, dtype=np.int64)
    k = nodes.size
    a, b = np.triu_indices(k, 1)
    keep = rng.random(a.size) < p
    return np.stack([nodes[a[keep]], nodes[b[keep]]], axis=1)


def _path_pairs(order):
    order = np.asarray(order, dtype=np.int64)
    return np.stack([order[:-1], order[1:]], axis=1)


def hub(n, p, hubs, q=0.2, sigma=0.1, seed=0):
    """ER(n, p), a Hamiltonian path 1-2-...-n (connectivity at small p), and every node of ``hubs`` adjacent to everyone."""
    rng = np.random.default_rng(seed)
    pairs = [_er_pairs(rng, np.arange(1, n + 1), p), _path_pairs(np.arange(1, n + 1))]
    for h in hubs:
        others = np.arange(1, n + 1); others = others[others != h]
        pairs.append(np.stack([np.full(n - 1, h), others], axis=1))
    return _measure(n, np.concatenate(pairs), q, sigma, rng)


def band(n, k, q=0.2, sigma=0.1, seed=0, chords=()):
    """i ~ i +- 1 .. +- k.  k = 1: the path.  ``chords``: further (i, j) pairs."""
    rng = np.random.default_rng(seed)
    i = np.arange(1, n + 1)
    pairs = [np.stack([i[:-d], i[d:]], axis=1) for d in range(1, k + 1)]
    if len(chords):
        pairs.append(np.asarray(chords, dtype=np.int64).reshape(-1, 2))
    return _measure(n, np.concatenate(pairs), q, sigma, rng)


def book(pages, q=0.2, sigma=0.1, seed=0):
    """The spine {1, 2} and ``pages`` triangles on it: every page k = 3 .. pages + 2 is adjacent to 1 and to 2.  The spine has codegree
    ``pages``, every page edge codegree 1 (its only cycle runs through the spine): n = pages + 2, m = 2 pages + 1."""
    rng = np.random.default_rng(seed)
    k = np.arange(3, pages + 3)
    pairs = [np.array([[1, 2]]), np.stack([np.full(pages, 1), k], axis=1), np.stack([np.full(pages, 2), k], axis=1)]
    return _measure(pages + 2, np.concatenate(pairs), q, sigma, rng)


def star(n, hub_id, q=0.2, sigma=0.1, seed=0):
    rng = np.random.default_rng(seed)
    others = np.arange(1, n + 1); others = others[others != hub_id]
    return _measure(n, np.stack([np.full(n - 1, hub_id), others], axis=1), q, sigma, rng)


def bipartite(a, b, p, q=0.2, sigma=0.1, seed=0):
    """Random bipartite graph on a + b nodes, the sides interleaved in the numbering (a random relabelling), made connected by a
    path that alternates between the sides as long as both last."""
    rng = np.random.default_rng(seed)
    n = a + b
    ids = rng.permutation(n) + 1
    A, B = ids[:a], ids[a:]
    ia, ib = np.nonzero(rng.random((a, b)) < p)
    pairs = [np.stack([A[ia], B[ib]], axis=1)]
    small, large = (A, B) if a <= b else (B, A)
    zig = np.empty(2 * small.size, dtype=np.int64); zig[0::2] = small; zig[1::2] = large[:small.size]
    pairs.append(_path_pairs(zig))
    rest = large[small.size:]
    if rest.size:
        pairs.append(np.stack([np.full(rest.size, small[0]), rest], axis=1))
    mo = _measure(n, np.concatenate(pairs), q, sigma, rng)
    side = np.zeros(n, dtype=bool); side[A - 1] = True
    mo.side = side
    return mo


def bridged(n1, n2, p1, p2, bridges, q=0.2, sigma=0.1, seed=0):
    """ER(n1, p1) on ids 1..n1 and ER(n2, p2) on n1+1..n1+n2, each with its Hamiltonian path, joined by ``bridges`` edges whose
    endpoints are distinct on both sides -- so no bridge lies on a 3-cycle.  ``mo.bridge`` marks them in ``Ind``'s order."""
    rng = np.random.default_rng(seed)
    n = n1 + n2
    left, right = np.arange(1, n1 + 1), np.arange(n1 + 1, n + 1)
    bl = rng.choice(left[n1 // 3:], bridges, replace=False)          # not the first rows: the bridges sit inside the edge list
    br = rng.choice(right, bridges, replace=False)
    pairs = [_er_pairs(rng, left, p1), _path_pairs(left), _er_pairs(rng, right, p2), _path_pairs(right), np.stack([bl, br], axis=1)]
    mo = _measure(n, np.concatenate(pairs), q, sigma, rng)
    mo.bridge = (mo.Ind[:, 0] <= n1) & (mo.Ind[:, 1] > n1)
    return mo


def power_law(n, avg, gamma, q=0.2, sigma=0.1, seed=0):
    """Chung-Lu: P(i ~ j) = min(1, w_i w_j / sum w) with w_i ~ (i + i0)^(-1 / (gamma - 1)) scaled to the average ``avg``, under a
    random relabelling, plus a Hamiltonian path in the new numbering."""
    rng = np.random.default_rng(seed)
    w = (np.arange(n) + 1.0) ** (-1.0 / (gamma - 1.0))
    w *= avg * n / w.sum()
    P = np.minimum(1.0, np.outer(w, w) / w.sum())
    a, b = np.triu_indices(n, 1)
    keep = rng.random(a.size) < P[a, b]
    ids = rng.permutation(n) + 1
    pairs = [np.stack([ids[a[keep]], ids[b[keep]]], axis=1), _path_pairs(np.arange(1, n + 1))]
    return _measure(n, np.concatenate(pairs), q, sigma, rng)


def dense_with_pendants(n, p, pendants, q=0.2, sigma=0.1, seed=0):
    """ER(n - pendants, p) on a random subset of the ids; the other ``pendants`` ids hang on it by one edge (the 1st, 3rd, ... of them) or by two
    (the 2nd, 4th, ...): degrees 1 and 2 among rows of hundreds."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(n) + 1
    core, pend = ids[:n - pendants], ids[n - pendants:]
    pairs = [_er_pairs(rng, core, p), _path_pairs(core)]
    for t, v in enumerate(pend):
        for u in rng.choice(core, 1 + t % 2, replace=False):
            pairs.append(np.array([[v, u]]))
    return _measure(n, np.concatenate(pairs), q, sigma, rng)


def two_components(n_small, n_large, p, q=0.1, sigma=0.05, seed=0):
    """For IRLS only: a small piece on ids 1..n_small (it holds node 1) and a larger one on the ids after it."""
    rng = np.random.default_rng(seed)
    a, b = np.arange(1, n_small + 1), np.arange(n_small + 1, n_small + n_large + 1)
    pairs = [_er_pairs(rng, a, p), _path_pairs(a), _er_pairs(rng, b, p), _path_pairs(b)]
    return _measure(n_small + n_large, np.concatenate(pairs), q, sigma, rng)


# ---- plain NumPy facts about a graph, from Ind alone ----------------------------------------------------------------------------
def degrees(Ind):
    n = int(Ind.max())
    return np.bincount(Ind.reshape(-1) - 1, minlength=n)


def codegrees(Ind):
    """Common neighbours of every edge's endpoints, (m,)."""
    n = int(Ind.max())
    A = np.zeros((n, n), dtype=bool)
    A[Ind[:, 0] - 1, Ind[:, 1] - 1] = True; A |= A.T
    out = np.empty(Ind.shape[0], dtype=np.int64)
    for a in range(0, Ind.shape[0], 4096):
        out[a:a + 4096] = (A[Ind[a:a + 4096, 0] - 1] & A[Ind[a:a + 4096, 1] - 1]).sum(axis=1)
    return out


def bfs_levels(Ind, root=1):
    """Level of every node from ``root`` (-1: not reached)."""
    n = int(Ind.max())
    order = np.argsort(np.concatenate([Ind[:, 0], Ind[:, 1]]), kind="stable")
    nbr = np.concatenate([Ind[:, 1], Ind[:, 0]])[order] - 1
    ptr = np.searchsorted(np.concatenate([Ind[:, 0], Ind[:, 1]])[order], np.arange(1, n + 2))
    level = np.full(n, -1, dtype=np.int64); level[root - 1] = 0
    front = np.array([root - 1])
    while front.size:
        nxt = np.unique(np.concatenate([nbr[ptr[v]:ptr[v + 1]] for v in front]))
        nxt = nxt[level[nxt] < 0]
        level[nxt] = level[front[0]] + 1
        front = nxt
    return level


def is_bipartite(Ind):
    lv = bfs_levels(Ind)
    return bool((lv >= 0).all() and ((lv[Ind[:, 0] - 1] + lv[Ind[:, 1] - 1]) % 2 == 1).all())


def first_round_chain_depth(Ind, S):
    """Boruvka's first round with the order (fl(S + 1), edge index): every node hooks under the other end of its lightest edge (of a
    mutual pair the smaller id stays the root).  Returns the longest chain of hooks -- what pointer jumping has to flatten."""
    n, m = int(Ind.max()), Ind.shape[0]
    rank = np.empty(m, dtype=np.int64); rank[np.lexsort((np.arange(m), np.asarray(S, dtype=np.float64) + 1.0))] = np.arange(m)
    best = np.full(n, m, dtype=np.int64)
    for c in (0, 1):
        np.minimum.at(best, Ind[:, c] - 1, rank)
    e = np.argsort(rank)[best]                                              # each node's lightest edge
    other = np.where(Ind[e, 0] - 1 == np.arange(n), Ind[e, 1] - 1, Ind[e, 0] - 1)
    parent = other.copy()
    v = np.arange(n)
    mutual = (other[other] == v) & (v < other)
    parent[mutual] = v[mutual]
    depth = np.zeros(n, dtype=np.int64); cur = parent.copy(); at = v.copy()
    for _ in range(n):
        move = cur != at
        if not move.any():
            break
        depth[move] += 1
        at = np.where(move, cur, at); cur = parent[at]
    return int(depth.max())


# ---- the solver of the Lie-algebraic averaging steps, restated -------------------------------------------------------------------
def jacobi_pcg(Ind, w, rhs, tol=1e-13, cap=None):
    """Jacobi-preconditioned CG on the grounded normal equations  A' W^2 A x = rhs  (node 1's unknown fixed at 0, as
    desc_amd/csrc/laa.hip: k_cg_lap), stop |r| <= tol |b|, cap min(20000, 20 n + 200).  rhs: (n, c).  -> (x, iterations of the
    slowest column)."""
    n = int(Ind.max())
    i, j = Ind[:, 0] - 1, Ind[:, 1] - 1
    w2 = np.asarray(w, dtype=np.float64) ** 2
    cap = min(20000, 20 * n + 200) if cap is None else cap
    diag = np.bincount(i, w2, n) + np.bincount(j, w2, n)

    def lap(p):
        d = w2[:, None] * (p[i] - p[j])
        q = np.zeros_like(p)
        np.add.at(q, i, d); np.add.at(q, j, -d)
        q[0] = 0
        return q

    b = np.array(rhs, dtype=np.float64); b[0] = 0
    x = np.zeros_like(b); r = b.copy()
    z = r / diag[:, None]; z[0] = 0
    p = z.copy()
    rz = np.sum(r * z, axis=0)
    bn = np.linalg.norm(b, axis=0)
    done = np.zeros(b.shape[1], dtype=bool); iters = np.zeros(b.shape[1], dtype=np.int64)
    for it in range(1, cap + 1):
        q = lap(p)
        alpha = np.where(done, 0.0, rz / np.where(done, 1.0, np.sum(p * q, axis=0)))
        x += alpha * p; r -= alpha * q
        done_now = np.linalg.norm(r, axis=0) <= tol * bn
        iters[~done & done_now] = it
        done |= done_now
        if done.all():
            return x, int(iters.max())
        z = r / diag[:, None]; z[0] = 0
        rz_new = np.sum(r * z, axis=0)
        p = z + np.where(done, 0.0, rz_new / np.where(done, 1.0, rz)) * p
        rz = rz_new
    return x, cap + 1


# ---- the table ------------------------------------------------------------------------------------------------------------------
# name -> (generator call, the branch sides the shape is there for (tests/test_graph_shapes.py: SIDES), the GPU tests that use it).
# tests/test_graph_shapes.py qualifies every row on the CPU; tests/test_gpu_graph_shapes.py runs them.
# The shapes CEMP's SVec is compared on carry noise but no outliers (q = 0): one Haar outlier cycle in ~1e4 has an angle within 1e-4 of
# pi, where acos turns 1 ulp of the trace into 1e-12 of S0 -- the oracle's own conditioning, not the kernel's (figures: QUALIFIED).
SHAPES = {
    # CEMP's LDS classes: 80 max_deg bytes of staged rotation blocks, 8 BI max_deg bytes of band rows
    "hub300_mid": (lambda: hub(300, 0.1, [150], q=0.0, sigma=0.2, seed=1),
                   ["s0_staged_default", "bi_partial", "hub_row_middle", "device_sampler", "every_edge_has_cycles"], ["cemp"]),
    "hub900_first": (lambda: hub(900, 0.02, [1], q=0.0, sigma=0.2, seed=20), ["s0_staged_optin", "bi_partial", "hub_row_first"], ["cemp"]),
    "hub2000_mid": (lambda: hub(2000, 0.005, [1000], q=0.0, sigma=0.3, seed=50), ["s0_plain_over_lds", "bi_partial", "hub_row_middle"], ["cemp"]),
    "hub2100_last": (lambda: hub(2100, 0.005, [2100], q=0.0, sigma=0.3, seed=51), ["s0_plain_over_lds", "bi_one", "hub_row_last"], ["cemp"]),
    "hub8300_mid": (lambda: hub(8300, 0.001, [4000], q=0.0, sigma=0.3, seed=51), ["s0_plain_tiles_off", "tiles_off_by_lds", "hub_row_middle"], ["cemp"]),
    "hubs4100_adjacent": (lambda: hub(4100, 0.001, [1, 2], q=0.0, sigma=0.3, seed=51), ["host_sampler", "s0_plain_tiles_off"], ["cemp", "lp_refusal"]),
    "hubs1100_adjacent": (lambda: hub(1100, 0.01, [1, 2], seed=7), ["device_builder_refuses", "device_sampler"], ["pgd_fallback"]),
    "hub1500_mid": (lambda: hub(1500, 0.01, [700], seed=19), ["one_row_far_longer", "device_builder_builds"], ["pgd"]),
    # the LAA core (refinement, MPLS, IRLS): which row is the long one
    "hub400_first": (lambda: hub(400, 0.05, [1], q=0.0, sigma=0.2, seed=8), ["hub_is_grounded_node", "long_row"], ["mpls"]),
    "hub400_last": (lambda: hub(400, 0.05, [400], q=0.0, sigma=0.2, seed=9), ["hub_is_last_node", "long_row"], ["mpls"]),
    # ... with outliers: the refinement started from GCW stops after one step without them
    "hub400_first_outliers": (lambda: hub(400, 0.05, [1], q=0.3, sigma=0.2, seed=8), ["hub_is_grounded_node", "long_row"], ["refine"]),
    "hub400_last_outliers": (lambda: hub(400, 0.05, [400], q=0.3, sigma=0.2, seed=9), ["hub_is_last_node", "long_row"], ["refine"]),
    "hub150_first": (lambda: hub(150, 0.1, [1], q=0.1, sigma=0.05, seed=40), ["hub_is_grounded_node"], ["irls"]),
    "power_law200": (lambda: power_law(200, 10, 2.5, q=0.1, sigma=0.05, seed=41), ["long_row"], ["irls"]),
    "band200_10_low_noise": (lambda: band(200, 10, q=0.0, sigma=0.1, seed=63), ["uniform_narrow_rows"], ["irls"]),
    # Spectral / GCW: a wave per row meeting one row of 599 slots
    "hub600_first": (lambda: hub(600, 0.03, [1], seed=10), ["wave_per_row_long_row", "not_bipartite"], ["spectral", "gcw"]),
    "hub600_last": (lambda: hub(600, 0.03, [600], seed=11), ["wave_per_row_long_row"], ["spectral", "gcw"]),
    "dense_pendants": (lambda: dense_with_pendants(450, 0.6, 6, seed=17), ["wg_per_row_short_row"], ["spectral", "gcw"]),
    "band200_10": (lambda: band(200, 10, q=0.0, sigma=0.2, seed=12), ["uniform_narrow_rows", "bi_full", "empty_tiles"],
                   ["cemp", "mpls", "refine", "spectral", "gcw"]),
    "star200_mid": (lambda: star(200, 100, seed=13), ["no_edge_has_cycles", "bipartite"], ["cemp", "spectral", "gcw"]),
    "bipartite60_90": (lambda: bipartite(60, 90, 0.3, seed=14), ["no_edge_has_cycles", "bipartite"], ["cemp", "spectral", "gcw"]),
    "bridged150_60": (lambda: bridged(150, 60, 0.3, 0.5, 5, q=0.0, sigma=0.2, seed=70), ["no_cycle_edges_inside", "bi_full"],
                      ["cemp", "mpls", "refine", "spectral", "gcw"]),
    # the LP: small enough that 50 PDHG steps of the restatement move by less than 1e-14 under 1 ulp of the rotations
    "hub100_mid": (lambda: hub(100, 0.15, [50], q=0.0, sigma=0.3, seed=80), ["every_edge_has_cycles", "hub_row_middle"], ["lp"]),
    "bridged50_30": (lambda: bridged(50, 30, 0.4, 0.6, 3, q=0.0, sigma=0.3, seed=80), ["no_cycle_edges_inside"], ["lp"]),
    "power_law500": (lambda: power_law(500, 12, 2.5, q=0.0, sigma=0.2, seed=16), ["no_cycle_edges_inside", "long_row"],
                     ["mpls", "refine", "spectral", "gcw", "pgd"]),
    "hub40_mid": (lambda: hub(40, 0.2, [20], q=0.0, sigma=0.2, seed=21), ["bi_full"], ["cemp_nsample"]),
    "two_components": (lambda: two_components(20, 60, 0.3, seed=18), ["largest_component_without_node_1"], ["irls"]),
}
_models = {}


def model(name):
    """The shape's model struct, built once per process."""
    if name not in _models:
        _models[name] = SHAPES[name][0]()
    return _models[name]


def shapes_for(use):
    return [k for k, v in SHAPES.items() if use in v[2]]


def noisy_truth(mo, seed):
    """The synthetic S_vec of tests/test_gpu_spectral.py: the true corruption levels plus noise, clipped to [2e-3, 1]."""
    rng = np.random.default_rng(seed)
    return np.clip(mo.ErrVec + 0.02 * rng.standard_normal(mo.ErrVec.shape), 2e-3, 1)


def ulp_perturbed(a, seed):
    """Every entry scaled by 1 + 2.2e-16 {-1, 0, 1}: what two correctly rounded evaluations can leave between them."""
    rng = np.random.default_rng(seed)
    return np.asarray(a) * (1.0 + 2.2e-16 * rng.integers(-1, 2, np.shape(a)))

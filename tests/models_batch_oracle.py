"""NumPy restatement of the batched generators' definition (include/desc_amd.h, "batched problem generator"): keys on uint64 arrays,
the uniform and normal draws, the streams, Uniform_Topology and Nonuniform_Topology with keyed selections.  Independent of the library:
nothing here imports desc_amd.  The projection is LAPACK's SVD; ``gap`` records how well conditioned each projection was, so that a test
can leave the ill-conditioned blocks out of a comparison with another SVD.

Blocks are stacks (count, 3, 3) with block[k][r, c] = entry (r, c); the library's 3 x 3 x count Fortran arrays are
``np.transpose(stack, (1, 2, 0))``."""
from types import SimpleNamespace

import numpy as np

U64 = np.uint64
STREAM = dict(edge=1, rorig=2, rcorr=3, corrupt=4, noise=5, haar=6, node=7, select=8, r0=9)      # DESC_MODELS_STREAM_*
TWO_PI = 6.283185307179586


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=U64))


def mix64(x):
    """splitmix64's finaliser on a uint64 array (wrapping multiplication)."""
    x = _u64(x).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U64(30); x *= U64(0xBF58476D1CE4E5B9)
        x ^= x >> U64(27); x *= U64(0x94D049BB133111EB)
        x ^= x >> U64(31)
    return x


def sample_key(seed, edge, k):
    """desc_sample_key on arrays."""
    with np.errstate(over="ignore"):
        a = mix64(_u64(seed) ^ ((_u64(edge) + U64(1)) * U64(0x9E3779B97F4A7C15)))
        return mix64(a ^ ((_u64(k) + U64(1)) * U64(0xD1B54A32D192ED03)))


def key(seed, stream, sub, ids, c):
    """desc_models_key(seed, stream, sub, id, c) for an array of ids."""
    return sample_key(sample_key(seed, stream, sub), ids, c)


def uniform(seed, stream, sub, ids, c=0):
    return (key(seed, stream, sub, ids, c) >> U64(11)).astype(np.float64) * 2.0 ** -53


def normal(seed, stream, sub, ids, c):
    k1, k2 = key(seed, stream, sub, ids, 2 * c), key(seed, stream, sub, ids, 2 * c + 1)
    u1 = ((k1 >> U64(12)).astype(np.float64) + 0.5) * 2.0 ** -52
    u2 = (k2 >> U64(11)).astype(np.float64) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)


def normal_blocks(seed, stream, sub, ids):
    """(len(ids), 3, 3): component c is entry (c mod 3, c div 3)."""
    ids = _u64(ids)
    out = np.zeros((ids.size, 3, 3))
    for c in range(9):
        out[:, c % 3, c // 3] = normal(seed, stream, sub, ids, c)
    return out


def project(Q):
    """U diag(1, 1, det(U V')) V' of a stack, and each block's gap: s2 + s3 when det(Q) > 0, else s2 - s3."""
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 3, 3)
    if Q.shape[0] == 0:
        return Q.copy(), np.zeros(0)
    Um, s, Vt = np.linalg.svd(Q)
    d = np.linalg.det(Um @ Vt)
    Um = Um.copy()
    Um[:, :, 2] *= d[:, None]
    gap = np.where(d > 0, s[:, 1] + s[:, 2], s[:, 1] - s[:, 2])
    return Um @ Vt, gap


def abs_acos_ext(x):
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    inside = np.abs(x) <= 1
    out[inside] = np.arccos(x[inside])
    out[x > 1] = np.arccosh(x[x > 1])
    out[x < -1] = np.hypot(np.pi, np.arccosh(-x[x < -1]))
    return out


def graph(n, p, seed):
    """0-based (i, j), i < j, sorted by (i, j): pair t is an edge iff its uniform draw is below p."""
    i, j = np.triu_indices(n, 1)                                 # row after row: t = i n - i (i + 1) / 2 + (j - i - 1) ascending
    t = i.astype(np.int64) * n - i.astype(np.int64) * (i + 1) // 2 + (j - i - 1)
    assert (t == np.arange(t.size)).all()
    keep = uniform(seed, STREAM["edge"], 0, t) < p
    return i[keep].astype(np.int64), j[keep].astype(np.int64)


def _finish(n, ii, jj, R, Rij_orig, R_orig, corrupted, gap, seed):
    tr = np.einsum("krc,krc->k", Rij_orig, R)
    return SimpleNamespace(n=n, Ind=np.stack([ii + 1, jj + 1], axis=1), RijMat=R, Rij_orig=Rij_orig, R_orig=R_orig,
                           ErrVec=abs_acos_ext((tr - 1.0) / 2.0) / np.pi, corrupted=corrupted, gap=gap, seed=seed)


def _mul_abt(A, B):
    return A @ np.transpose(B, (0, 2, 1))


def uniform_topology(n, p, q, sigma, model="uniform", seed=0):
    ii, jj = graph(n, p, seed)
    m = ii.size
    e = np.arange(m)
    R_orig, g_orig = project(normal_blocks(seed, STREAM["rorig"], 0, np.arange(n)))
    R_corr, g_corr = project(normal_blocks(seed, STREAM["rcorr"], 0, np.arange(n)))
    Rij_orig = _mul_abt(R_orig[ii], R_orig[jj])
    gap = np.minimum(g_orig[ii], g_orig[jj])
    noise = uniform(seed, STREAM["corrupt"], 0, e) >= q if m else np.zeros(0, bool)
    N = normal_blocks(seed, STREAM["noise"], 0, e)
    Q = Rij_orig + sigma * N
    bad = ~noise
    if model == "uniform":
        Q[bad] = normal_blocks(seed, STREAM["haar"], 0, e[bad])
    else:
        Q[bad] = _mul_abt(R_corr[ii[bad]], R_corr[jj[bad]]) + sigma * N[bad]
        gap[bad] = np.minimum(gap[bad], np.minimum(g_corr[ii[bad]], g_corr[jj[bad]]))
    R, g = project(Q)
    return _finish(n, ii, jj, R, Rij_orig, R_orig, bad, np.minimum(gap, g), seed)


def corrupted_nodes(n, p_node_crpt, seed):
    """The corrupted nodes in node order (ascending (key, id))."""
    kv = key(seed, STREAM["node"], 0, np.arange(n), 0)
    order = np.lexsort((np.arange(n), kv))
    return order[: int(np.floor(n * p_node_crpt))]


def selections(n, ii, jj, p_node_crpt, p_edge_crpt, seed):
    """winner[e]: the node whose selection of edge e stands (-1: nobody selected it)."""
    winner = np.full(ii.size, -1, dtype=np.int64)
    for v in corrupted_nodes(n, p_node_crpt, seed):                   # a later node overwrites an earlier one
        inc = np.flatnonzero((ii == v) | (jj == v))
        ke = key(seed, STREAM["select"], v, inc, 0)
        chosen = inc[np.lexsort((inc, ke))][: int(np.floor(p_edge_crpt * inc.size))]
        winner[chosen] = v
    return winner


def nonuniform_topology(n, p, p_node_crpt, p_edge_crpt, sigma_in, sigma_out, crpt_type="uniform", seed=0):
    assert crpt_type in ("uniform", "self-consistent", "adv")
    ii, jj = graph(n, p, seed)
    m = ii.size
    e = np.arange(m)
    R_orig, g_orig = project(normal_blocks(seed, STREAM["rorig"], 0, np.arange(n)))
    R_crpt, g_crpt = project(normal_blocks(seed, STREAM["rcorr"], 0, np.arange(n)))
    Rij_orig = _mul_abt(R_orig[ii], R_orig[jj])
    gap = np.minimum(g_orig[ii], g_orig[jj])
    winner = selections(n, ii, jj, p_node_crpt, p_edge_crpt, seed)
    base = Rij_orig.copy()
    for k in np.flatnonzero(winner >= 0):
        w = int(winner[k])
        first = w == ii[k]
        x = int(jj[k] if first else ii[k])
        if crpt_type == "uniform":
            M, g = project(normal_blocks(seed, STREAM["r0"], w, [k]))
            M, gap[k] = M[0], min(gap[k], g[0])
        elif crpt_type == "self-consistent":
            M = R_crpt[w] @ R_crpt[x].T
            gap[k] = min(gap[k], g_crpt[w], g_crpt[x])
        else:
            M = R_crpt[w] @ R_orig[x].T
            gap[k] = min(gap[k], g_crpt[w], g_orig[x])
        base[k] = M if first else M.T
    bad = winner >= 0
    sig = np.where(bad, sigma_out, sigma_in)
    R, g = project(base + sig[:, None, None] * normal_blocks(seed, STREAM["noise"], 0, e))
    out = _finish(n, ii, jj, R, Rij_orig, R_orig, bad, np.minimum(gap, g), seed)
    out.winner = winner
    return out

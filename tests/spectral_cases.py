"""TEST INFRASTRUCTURE -- the inputs of the kernel-by-kernel tests of the Spectral / GCW eigen-solve (tests/test_gpu_spectral_kernels.py,
tests/test_spectral_host.py, tests/test_gpu_spectral_exits.py): small graphs whose CSR rows sit on the slot-count edges of k_bsr_spmm,
operands, and the matrices of the small dense helpers.  Everything is seeded; nothing here touches the library."""
import functools

import numpy as np

from tests.graph_shapes import _er_pairs

BW = 6
# leaves per star: the edges of k_bsr_spmm<TPR>'s row loop `for (t = r0 + tr; t < r1; t += 2 TPR) { two = t + TPR < r1; ... }` --
# TPR - 1, TPR, TPR + 1 (the second slot of a lane appears), 2 TPR - 1, 2 TPR, 2 TPR + 1 (the second pass appears), and a row between
LEAVES_64 = (0, 1, 63, 64, 65, 127, 128, 129, 200)
LEAVES_256 = (255, 256, 257, 511, 512, 513)
GRIDS = (1, 3, 0)             # forced workgroup counts; 0: the product path's rule
S_VALUES = (0.0, 1e-300, 2e-3, 1.0, 1e6, float("inf"), -1.0, float("nan"))
ROW_COUNTS = (1, 3, 255, 256, 257, 65535, 65536, 65537)      # 65536 = 256 workgroups x 256 threads: the first count at which a thread strides


def haar(rng, count):
    q, r = np.linalg.qr(rng.standard_normal((count, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def _problem(n, pairs, seed):
    """pairs: 0-based (i, j) -> (n, ii, jj, rij (m, 9) with component r + 3c), i < j, sorted by (i, j), Haar rotations."""
    P = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    P = np.unique(np.sort(P[P[:, 0] != P[:, 1]], axis=1), axis=0)
    R = haar(np.random.default_rng(seed), P.shape[0])
    rij = np.ascontiguousarray(np.transpose(R, (0, 2, 1)).reshape(-1, 9))          # [e, 3c + r] = R[e, r, c]
    return n, P[:, 0].astype(np.int32), P[:, 1].astype(np.int32), rij


@functools.lru_cache(maxsize=None)
def star_forest(leaves, seed=11):
    """One star per entry L of `leaves`, on L + 1 consecutive node ids with the centre in the middle of its leaves (its row then holds
    slots with v > u, the transposed branch of assembly, and slots with v < u); L = 0 is an isolated node.
    -> (n, ii, jj, rij, centres)."""
    pairs, centres, base = [], [], 0
    for L in leaves:
        c = base + L // 2
        centres.append(c)
        pairs += [(c, u) for u in range(base, base + L + 1) if u != c]
        base += L + 1
    n, ii, jj, rij = _problem(base, np.array(pairs, dtype=np.int64).reshape(-1, 2), seed)
    return n, ii, jj, rij, tuple(centres)


@functools.lru_cache(maxsize=None)
def er_graph(n=60, p=0.3, seed=12):
    rng = np.random.default_rng(seed)
    pairs = _er_pairs(rng, np.arange(1, n + 1), p) - 1
    return _problem(n, pairs, seed + 1)


@functools.lru_cache(maxsize=None)
def tiny_graph(n):
    """A path on n nodes (n = 1: no edge), for the row sums."""
    return _problem(n, np.array([(i, i + 1) for i in range(n - 1)], dtype=np.int64).reshape(-1, 2), 20 + n)


def graphs():
    """name -> (n, ii, jj, rij)"""
    return {"stars64": star_forest(LEAVES_64)[:4], "stars256": star_forest(LEAVES_256)[:4], "er60": er_graph()}


def operand(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(3 * n, BW))


def edge_weights(m, kind, seed=3):
    """unit: None; wide: 10^U(-8, 8)."""
    if kind == "unit":
        return None
    return 10.0 ** np.random.default_rng(seed).uniform(-8.0, 8.0, size=m)


def dinv_with_zeros(n, seed=4):
    rng = np.random.default_rng(seed)
    d = 1.0 / np.sqrt(rng.uniform(0.5, 50.0, size=n))
    d[rng.random(n) < 0.2] = 0.0
    d[0] = 0.0
    return d


def spmm_params():
    """name -> (alpha, s1, s2, z: 'x' | 'other' | 'nan', z_is_y).  cheb1 / cheb2 are the first and a later step of the Chebyshev
    recurrence of spectral_impl for lo = -1, cut = 0.3, top = 0.9: e = (cut - lo) / 2, c = (cut + lo) / 2, s_prev = e / (top - c)."""
    e, c = 0.65, -0.35
    s_prev = e / (0.9 - c)
    s_new = 1.0 / (2.0 / s_prev - s_prev)
    return {
        "plain": (1.0, 0.0, 0.0, "x", False),
        "cheb1": (s_prev / e, -c * s_prev / e, 0.0, "x", False),
        "cheb2": (2.0 * s_new / e, -2.0 * s_new * c / e, -s_prev * s_new, "other", False),
        "nan_z": (1.25, -0.5, 0.0, "nan", False),
        "z_is_y": (2.0 * s_new / e, -2.0 * s_new * c / e, -s_prev * s_new, "other", True),
    }


def residual_near_eigenpair(rows, seed=8):
    """X with orthonormal columns, Y = X diag(lam) + 1e-12 |lam| E: the explicit residual is ~1e-12 |lam| |E z|, where the Gram form
    z'G2 z - theta^2 has lost every digit (1e-24 against rounding of 1e-16)."""
    rng = np.random.default_rng(seed)
    X = np.linalg.qr(rng.standard_normal((rows, 6)))[0]
    lam = np.array([25.0, 24.0, 23.5, 8.0, 7.0, 6.0])
    E = rng.standard_normal((rows, 6)) / np.sqrt(rows)
    return X, X * lam + 1e-12 * 25.0 * E, np.eye(6)[:, :3].copy(), lam[:3].copy()



# ------------------------------------------------------------------------------------------------------------------ small dense helpers
def _rot(rng):
    return haar(rng, 1)[0]


SIGMA3 = (1.0, 1e-2, 1e-4, 1e-6, 1e-7, 1e-8, 1e-9, 1e-11, 1e-13, 0.0)


def project_cases(per_rung=12, seed=5):
    """name -> (count, 3, 3) blocks: the condition ladder M = U diag(1, 0.7, +-sigma_3) V' at both signs of the determinant, exact
    rank 2, rank 1 and zero, the scales 1e-100 and 1e100, exact rotations."""
    rng = np.random.default_rng(seed)
    out = {}
    for s3 in SIGMA3:
        for sg, tag in ((1.0, "+"), (-1.0, "-")):
            out[f"ladder{tag}{s3:g}"] = np.stack([_rot(rng) @ np.diag([1.0, 0.7, sg * s3]) @ _rot(rng).T for _ in range(per_rung)])
    a, b, c, d = (rng.standard_normal((per_rung, 3)) for _ in range(4))
    out["rank2"] = a[:, :, None] * b[:, None, :] + c[:, :, None] * d[:, None, :]             # exactly rank 2 only up to rounding ...
    r2 = np.zeros((per_rung, 3, 3)); r2[:, 0, 0] = rng.uniform(0.5, 2, per_rung); r2[:, 1, 2] = rng.uniform(0.5, 2, per_rung)
    r2[:, 1, 1] = rng.uniform(-1, 1, per_rung)
    out["rank2_exact"] = r2                                                               # ... these have a zero row and a zero column
    out["rank2_small"] = np.stack([np.diag([1.0, 1e-9, 0.0]), np.diag([0.0, 3.0, 1e-12]), np.diag([1e-5, 0.0, 1.0])])
    ints = rng.integers(-4, 5, size=(per_rung, 2, 3)).astype(np.float64)
    ints[:, 0, 0] += 9
    out["rank1_exact"] = ints[:, 0, :, None] * ints[:, 1, None, :] + 0.0
    out["rank1_axis"] = np.stack([np.outer(np.eye(3)[i], np.eye(3)[j]) * s for i in range(3) for j in range(3) for s in (1.0, -2.5)])
    out["zero"] = np.zeros((1, 3, 3))
    base = np.stack([_rot(rng) @ np.diag([1.0, 0.7, 0.2]) @ _rot(rng).T for _ in range(per_rung)])
    out["scale1e-100"] = base * 1e-100
    out["scale1e100"] = base * 1e100
    out["rotation"] = np.concatenate([haar(rng, per_rung), np.eye(3)[None]])
    return out


def jacobi_cases(seed=6):
    """name -> list of square matrices (N = 3 or 6)."""
    rng = np.random.default_rng(seed)
    out = {}
    for N in (3, 6):
        S = rng.standard_normal((8, N, N))
        out[f"random{N}"] = list(S + np.transpose(S, (0, 2, 1)))
        out[f"diagonal{N}"] = [np.diag(rng.standard_normal(N)), np.diag(np.arange(N, dtype=np.float64))]
        out[f"equal{N}"] = [np.eye(N) * 2.5, np.diag([3.0, 3.0, 1.0] + [1.0] * (N - 3))]
        out[f"zero{N}"] = [np.zeros((N, N))]
        out[f"asymmetric{N}"] = list(rng.standard_normal((4, N, N)))
        Q = np.linalg.qr(rng.standard_normal((N, N)))[0]
        out[f"graded{N}"] = [Q @ np.diag(10.0 ** -np.arange(0, 2 * N, 2.0)) @ Q.T]
    return out


def ortho_good_cases(seed=7):
    """name -> (G, Z): G = Y'Y of a 40 x 6 block whose columns are scaled by up to 1e6 (cond(G) up to 1e12, the cap the filter
    enforces), Z the identity or an orthogonal matrix."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, scale in enumerate((1.0, 1e2, 1e4, 1e6)):
        Y = np.linalg.qr(rng.standard_normal((40, 6)))[0] @ (np.eye(6) + 0.3 * rng.standard_normal((6, 6)))
        Y = Y * np.geomspace(1.0, scale, 6)[rng.permutation(6)]
        G = Y.T @ Y
        out[f"scale{scale:g}_I"] = (G, None)
        out[f"scale{scale:g}_Z"] = (G, np.linalg.qr(rng.standard_normal((6, 6)))[0])
    return out


def ortho_bad_cases():
    """name -> G for which ortho_coeffs must answer false."""
    neg = np.eye(6); neg[2, 2] = -1.0
    nan = np.eye(6); nan[1, 1] = np.nan
    return {"zero": np.zeros((6, 6)), "rank3": np.diag([1.0, 1.0, 1.0, 0.0, 0.0, 0.0]), "negative": neg, "nan": nan}


# ------------------------------------------------------------------------------------------------------------------ exits
@functools.lru_cache(maxsize=None)
def exit_model():
    from desc_amd.models import Uniform_Topology
    return Uniform_Topology(60, 0.5, 0.2, 0.1, "uniform", seed=21)


def exit_problem():
    """-> (mo, n, ii, jj, rij (m, 9)) of exit_model()."""
    from desc_amd.algorithms import marshal_edges
    mo = exit_model()
    n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None
    return mo, n, ii, jj, rij.reshape(-1, 9)


def exit_inputs():
    """name -> (weights | None, S_vec | None, normalize_rows): the Spectral matrix, a weighted matrix without row normalisation, GCW."""
    mo = exit_model()
    m = mo.Ind.shape[0]
    rng = np.random.default_rng(22)
    S = np.clip(mo.ErrVec + 0.02 * rng.standard_normal(m), 2e-3, 1.0)
    return {"spectral": (None, None, False), "weighted": (rng.uniform(0.5, 2.0, size=m), None, False), "gcw": (None, S, True)}


def exit_dense(name):
    """-> (the symmetric dense matrix the eigen-solve iterates, sigma): sigma = 1 under row normalisation, else the largest weighted degree."""
    from tests import spectral_kernels_oracle as O
    w, S, norm = exit_inputs()[name]
    _, n, ii, jj, rij = exit_problem()
    if S is not None:
        w = 1.0 / (S ** 1.5 + 1e-8)
    deg = O.row_wsum(n, ii, jj, w)[0]
    dinv = 1.0 / np.sqrt(deg) if norm else None
    A = O.dense_from_blocks(n, ii, jj, O.assemble(n, ii, jj, rij, w, dinv))
    return A, (1.0 if norm else float(deg.max()))


def ritz_tail_cases(n=7, seed=9):
    """name -> (V (3n, 3), dinv | None): Ritz vectors whose node blocks are noisy multiples of rotations (cond ~ 1, as the eigen-solve
    produces them), with either sign of det(V(1:3, :)) -- the sign fix of Spectral.m:39 -- and with / without the D^-1/2 scaling."""
    rng = np.random.default_rng(seed)
    G = haar(rng, 1)[0]
    V = np.concatenate([(R @ G + 0.05 * rng.standard_normal((3, 3))) * s for R, s in zip(haar(rng, n), rng.uniform(0.5, 2.0, n))])
    if np.linalg.det(V[:3]) < 0:
        V[:, 0] = -V[:, 0]
    Vn = V.copy(); Vn[:, 0] = -Vn[:, 0]
    dinv = 1.0 / np.sqrt(rng.uniform(1.0, 40.0, n))
    return {"plain_pos": (V, None), "plain_neg": (Vn, None), "dinv_pos": (V, dinv), "dinv_neg": (Vn, dinv)}

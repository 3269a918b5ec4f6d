"""TEST INFRASTRUCTURE -- NumPy restatements of the kernels of the Spectral / GCW eigen-solve (desc_amd/csrc/spectral.hip), one per
kernel, for tests/test_gpu_spectral_kernels.py (the device side, through the desc_test_spectral_* hooks) and
tests/test_spectral_host.py (which qualifies these restatements against oracle/spectral_oracle.py without a GPU).

Two kinds of restatement:
  * bit-exact: the kernel's own operation order in float64 (assembly, k_combine) -- the device result must be equal bit for bit;
  * high precision: np.longdouble / mpmath on the same double inputs, with a first-order error bound that holds for ANY summation
    order (spmm, row sums, Gram matrices, residuals, weights).  The bounds are derived below, none is measured.

Layout, as the library stores it: the graph's CSR has every edge e = (i, j), i < j, in both endpoint rows, neighbours ascending; the
block of slot t in row v towards u is w_e dinv[v] dinv[u] (v < u ? R_e : R_e'), column-major 3x3, component q = r + 3k at
blocks[q, t].  x, y, z are (3n, 6) row-major."""
import math

import mpmath as mp
import numpy as np

EPS = 2.0 ** -53            # unit round-off of float64
BW = 6


def csr(n, ii, jj):
    """-> rowptr (n + 1), adj (2m), adj_eid (2m): neighbours ascending, the edge id of every slot (common.h: build_csr)."""
    ii, jj = np.asarray(ii, dtype=np.int64), np.asarray(jj, dtype=np.int64)
    m = ii.size
    src = np.concatenate([ii, jj]); dst = np.concatenate([jj, ii]); eid = np.concatenate([np.arange(m), np.arange(m)])
    order = np.lexsort((dst, src))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, src + 1, 1)
    return np.cumsum(rowptr), dst[order], eid[order]


def slots(n, ii, jj):
    rp = csr(n, ii, jj)[0]
    return rp[1:] - rp[:-1]


# ------------------------------------------------------------------------------------------------------------------ assembly
def assemble(n, ii, jj, rij, w=None, dinv=None):
    """k_assemble_blocks in float64 with its bracketing ((w * d_lo) * d_hi) * R[q], lo / hi = the smaller / larger node id of the edge:
    -> blocks (9, 2m).  rij: (m, 9), component r + 3c of R_e."""
    rp, adj, eid = csr(n, ii, jj)
    rij = np.asarray(rij, dtype=np.float64).reshape(-1, 9)
    m = rij.shape[0]
    w = np.ones(m) if w is None else np.asarray(w, dtype=np.float64)
    dinv = np.ones(n) if dinv is None else np.asarray(dinv, dtype=np.float64)
    row = np.repeat(np.arange(n), rp[1:] - rp[:-1])
    lo, hi = np.minimum(row, adj), np.maximum(row, adj)
    with np.errstate(all="ignore"):
        s = (w[eid] * dinv[lo]) * dinv[hi]
        Re = rij[eid]                                                   # (2m, 9)
        transposed = np.array([c + 3 * r for c in range(3) for r in range(3)])     # q = r + 3c  <-  R[c + 3r]
        Rt = Re[:, transposed]
        out = np.where((row < adj)[:, None], s[:, None] * Re, s[:, None] * Rt)
    return np.ascontiguousarray(out.T)


def dense_from_blocks(n, ii, jj, blocks):
    """The 3n x 3n matrix the stored blocks stand for."""
    rp, adj, _ = csr(n, ii, jj)
    A = np.zeros((3 * n, 3 * n), dtype=blocks.dtype)
    row = np.repeat(np.arange(n), rp[1:] - rp[:-1])
    for t in range(adj.size):
        v, u = row[t], adj[t]
        A[3 * v:3 * v + 3, 3 * u:3 * u + 3] = blocks[:, t].reshape(3, 3).T       # column-major component r + 3k
    return A


# ------------------------------------------------------------------------------------------------------------------ spmm
def spmm(n, ii, jj, blocks, x, z, alpha, s1, s2):
    """y = alpha A x + s1 x + s2 z in np.longdouble (the s2 term is left out when s2 == 0, as in the kernel: a NaN in z must not
    spread) -> (y as float64, bound).

    Bound per entry, first order, for any summation order: a row of `slots` blocks is a sum of 3 * slots products, each rounded once
    (eps |a x|), added in some tree (at most 3 * slots - 1 additions on any path, each eps of a partial sum <= sum |a x|); then three
    more roundings (alpha *, s1 x and s2 z products) and two additions.  So |err| <= (3 slots + 3) eps (|alpha| |A||x| + |s1 x| + |s2 z|).
    The longdouble reference's own error is 2^-11 of that."""
    L = np.longdouble
    rp, adj, _ = csr(n, ii, jj)
    x = np.asarray(x, dtype=np.float64).reshape(3 * n, BW)
    z = np.asarray(z, dtype=np.float64).reshape(3 * n, BW)
    Bl = blocks.astype(L).T.reshape(-1, 3, 3).transpose(0, 2, 1)                 # (2m, r, k)
    xb = x.astype(L).reshape(n, 3, BW)
    prod = np.einsum("trk,tkc->trc", Bl, xb[adj]) if adj.size else np.zeros((0, 3, BW), dtype=L)
    mag = np.einsum("trk,tkc->trc", np.abs(Bl), np.abs(xb[adj])) if adj.size else np.zeros((0, 3, BW), dtype=L)
    Ax = np.zeros((n, 3, BW), dtype=L); Am = np.zeros((n, 3, BW), dtype=L)
    row = np.repeat(np.arange(n), rp[1:] - rp[:-1])
    np.add.at(Ax, row, prod); np.add.at(Am, row, mag)
    Ax, Am = Ax.reshape(3 * n, BW), Am.reshape(3 * n, BW)
    y = L(alpha) * Ax + L(s1) * x.astype(L)
    size = abs(L(alpha)) * Am + np.abs(L(s1) * x.astype(L))
    if s2 != 0.0:
        y = y + L(s2) * z.astype(L)
        size = size + np.abs(L(s2) * z.astype(L))
    nslot = np.repeat(rp[1:] - rp[:-1], 3).astype(np.float64)[:, None]
    bound = ((3.0 * nslot + 3.0) * EPS) * size.astype(np.float64)
    return y.astype(np.float64), bound


# ------------------------------------------------------------------------------------------------------------------ weights, row sums
def gcw_weights(S):
    """1 / (S^1.5 + 1e-8) rounded once from 50 digits (1e-8 is the double the kernel adds); NaN for a negative or NaN S, 0 for +inf."""
    out = np.empty(len(S))
    with mp.workdps(60):
        c = mp.mpf(1e-8)
        for k, s in enumerate(np.asarray(S, dtype=np.float64)):
            if math.isnan(s) or s < 0:
                out[k] = math.nan
            elif math.isinf(s):
                out[k] = 0.0
            else:
                out[k] = float(1 / (mp.mpf(float(s)) ** mp.mpf(1.5) + c))
    return out


def row_wsum(n, ii, jj, w=None):
    """Weighted degrees, exactly rounded (math.fsum) -> (deg, bound).  Bound for any order: `slots` terms, at most slots - 1 additions
    on a path -- (slots + 4) eps sum |w| covers the 16-lane split and the four butterfly levels (4 = log2 16 additions more)."""
    rp, _, eid = csr(n, ii, jj)
    w = np.ones(len(ii)) if w is None else np.asarray(w, dtype=np.float64)
    deg = np.array([math.fsum(w[eid[rp[v]:rp[v + 1]]]) for v in range(n)])
    mag = np.array([math.fsum(np.abs(w[eid[rp[v]:rp[v + 1]]])) for v in range(n)])
    return deg, (rp[1:] - rp[:-1] + 4) * EPS * mag


# ------------------------------------------------------------------------------------------------------------------ gram, residual, combine
def gram(X, Y):
    """-> (X'Y, Y'Y, bound1, bound2) from np.longdouble.  A sum of `rows` products in any order: rows * eps * sum |x_a y_b|."""
    L = np.longdouble
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    rows = X.shape[0]
    G1 = (X.astype(L).T @ Y.astype(L)).astype(np.float64)
    G2 = (Y.astype(L).T @ Y.astype(L)).astype(np.float64)
    b1 = rows * EPS * (np.abs(X).astype(L).T @ np.abs(Y).astype(L)).astype(np.float64)
    b2 = rows * EPS * (np.abs(Y).astype(L).T @ np.abs(Y).astype(L)).astype(np.float64)
    return G1, G2, b1, b2


def residual(X, Y, Z3, theta):
    """sqrt(r2[c]) with r2[c] = |Y z_c - theta_c X z_c|^2 from np.longdouble -> (norms (3,), bound (3,)).

    Bound: row r's d = Y z - theta X z is two dot products of BW terms (BW roundings of products, BW - 1 additions), one product with
    theta and one subtraction: |err d_r| <= (BW + 3) eps (|Y_r||z| + |theta| |X_r||z|) =: e_r.  The norm of a vector moves by at most the
    norm of its perturbation, so sqrt(r2) moves by at most |e|_2; squaring and adding `rows` non-negative terms in any order is
    relative (rows + 1) eps on r2, i.e. half of that on the root: rows * eps * sqrt(r2) covers it."""
    L = np.longdouble
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    Z3, theta = np.asarray(Z3, dtype=np.float64).reshape(BW, 3), np.asarray(theta, dtype=np.float64).reshape(3)
    d = Y.astype(L) @ Z3.astype(L) - (X.astype(L) @ Z3.astype(L)) * theta.astype(L)
    nrm = np.sqrt((d * d).sum(axis=0)).astype(np.float64)
    e = (BW + 3) * EPS * (np.abs(Y) @ np.abs(Z3) + (np.abs(X) @ np.abs(Z3)) * np.abs(theta))
    return nrm, np.sqrt((e * e).sum(axis=0)) + X.shape[0] * EPS * nrm


def combine(Y, Cm):
    """k_combine in float64 in the kernel's order: s = 0; s += y[a] * C[a, b] for a = 0 .. 5."""
    Y, Cm = np.asarray(Y, dtype=np.float64), np.asarray(Cm, dtype=np.float64).reshape(BW, BW)
    out = np.zeros_like(Y)
    for b in range(BW):
        s = np.zeros(Y.shape[0])
        for a in range(BW):
            s = s + Y[:, a] * Cm[a, b]
        out[:, b] = s
    return out


# ------------------------------------------------------------------------------------------------------------------ small dense helpers
def project_numpy(M):
    """The body of oracle/spectral_oracle.py::_project for one block: U diag(1, 1, det(U V')) V' from LAPACK's SVD."""
    U, _, Vt = np.linalg.svd(M)
    return U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt


def project_exact(M):
    """The same projection from mpmath's SVD at 50 digits, rounded once."""
    with mp.workdps(50):
        U, _, V = mp.svd_r(mp.matrix(np.asarray(M, dtype=np.float64).tolist()))
        R = U * mp.diag([1, 1, mp.sign(mp.det(U * V))]) * V
        return np.array([[float(R[i, j]) for j in range(3)] for i in range(3)])


def so3_defect(R):
    """max(|R R' - I|, |det R - 1|)."""
    return max(float(np.abs(R @ R.T - np.eye(3)).max()), abs(float(np.linalg.det(R)) - 1.0))


def projection_is_unique(M):
    """sigma_2 + sign(det M) sigma_3 >= 1e-6 sigma_1: the nearest rotation is unique and well conditioned."""
    s = np.linalg.svd(M, compute_uv=False)
    if not s[0] > 0:
        return False
    sg = np.sign(np.linalg.det(M / s[0]))
    return bool(s[1] + sg * s[2] >= 1e-6 * s[0])


def projection_sensitivity(M, seed=0, trials=20):
    """The largest change of NumPy's own projection under `trials` random relative perturbations of size eps of M's entries."""
    rng = np.random.default_rng(seed)
    R0 = project_numpy(M)
    worst = 0.0
    for _ in range(trials):
        P = M * (1.0 + 2.0 * EPS * rng.choice([-1.0, 1.0], size=(3, 3)))
        worst = max(worst, float(np.abs(project_numpy(P) - R0).max()))
    return worst


def eig_defects(A, w, V):
    """(eigen-residual max |A V - V diag(w)|, orthogonality max |V'V - I|) for the symmetrised A."""
    A = 0.5 * (A + A.T)
    return float(np.abs(A @ V - V * w).max()), float(np.abs(V.T @ V - np.eye(A.shape[0])).max())


def ortho_defect(G, Cm):
    return float(np.abs(Cm.T @ G @ Cm - np.eye(G.shape[0])).max())


def ortho_numpy(G, Z=None):
    """A Cholesky-based C of NumPy: K = Z'GZ = L L', C = Z L^-T."""
    Z = np.eye(G.shape[0]) if Z is None else Z
    K = Z.T @ G @ Z
    Lc = np.linalg.cholesky(0.5 * (K + K.T))
    return Z @ np.linalg.solve(Lc, np.eye(G.shape[0])).T

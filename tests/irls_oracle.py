"""ORACLE -- test infrastructure only.  NumPy / SciPy restatement of Algorithms/IRLS_GM.m and IRLS_L12.m with the three Utils files
they call: BoxMedianSO3Graph.m (spanning-tree start, L1 loop, l1decode_pd), RobustMeanSO3Graph.m and L12.m.

* l1decode_pd forms the dense H11p = A' diag(sigx) A, solves it with scipy.linalg.lu_factor / lu_solve and estimates hcond with
  LAPACK's dgecon (1-norm), as MATLAB's linsolve does.
* The reweighted stage solves the weighted least squares by the normal equations A' W^2 A, formed with scipy.sparse and solved
  densely (Cholesky), so that C2 (N = 1000) runs in seconds.  MATLAB solves (W A) \\ (W B) by sparse QR.
* Largest component: of several of maximal size the one holding the smallest node id (graphconncomp's numbering is assumed).
PARITY UNPINNED by the reference: MATLAB cannot run here."""
import numpy as np
import scipy.linalg
import scipy.sparse
import scipy.sparse.csgraph

from oracle.refine_oracle import R2Q, q2R, qmul

EPS = np.finfo(np.float64).eps


def largest_component(Ind, N):
    """IRLS_GM.m:65-67 -> (nodes (0-based, ascending), edge mask)."""
    Ind = np.asarray(Ind, dtype=np.int64)
    G = scipy.sparse.coo_matrix((np.ones(Ind.shape[0]), (Ind[:, 0] - 1, Ind[:, 1] - 1)), shape=(N, N))
    _, lab = scipy.sparse.csgraph.connected_components(G, directed=False)
    size = np.bincount(lab)
    first = {}
    for v in range(N):
        first.setdefault(lab[v], v)
    best = None
    for l, v in sorted(first.items(), key=lambda t: t[1]):        # components by their smallest node: the first of maximal size
        if best is None or size[l] > size[best]:
            best = l
    nodes = np.flatnonzero(lab == best)
    return nodes, lab[Ind[:, 0] - 1] == best


def project(RR):
    """IRLS_GM.m:82-93 on RR (3 x 3 x m, already transposed): -> (projected RR, warned edge count).  Raises ValueError naming the
    1-based edge, as the reference's error()."""
    out = np.empty_like(RR)
    warned = 0
    for e in range(RR.shape[2]):
        d = np.linalg.det(RR[:, :, e])
        if d <= 0:
            raise ValueError(f"det(RR(:,:,{e + 1}))={d:f}")
        U, S, Vt = np.linalg.svd(RR[:, :, e])
        dev = np.abs(S - 1)
        if np.all(dev >= .1):                                      # MATLAB's if on a vector: all entries
            raise ValueError(f"svd(RR(:,:,{e + 1}))=[{S[0]:f} {S[1]:f} {S[2]:f}]")
        elif np.all(dev >= .01):
            warned += 1
        out[:, :, e] = U @ np.diag(np.round(S)) @ Vt
    return out, warned


def tree_start(I, QQ, N):
    """BoxMedianSO3Graph.m:78-114: passes over the columns of I in their order.  -> (Q N x 4, passes, tree edge sequence)."""
    Q = np.tile([1.0, 0, 0, 0], (N, 1))
    done = np.zeros(N, dtype=bool); done[0] = True
    passes, seq = 0, []
    while done.sum() < N:
        span = False
        passes += 1
        for j in range(I.shape[1]):
            a, b = I[0, j] - 1, I[1, j] - 1
            q = QQ[j]
            if done[a] and not done[b]:
                p = Q[a]
                Q[b] = [q[0] * p[0] - (q[1] * p[1] + q[2] * p[2] + q[3] * p[3]),
                        q[0] * p[1] + p[0] * q[1] + (q[2] * p[3] - q[3] * p[2]),
                        q[0] * p[2] + p[0] * q[2] + (q[3] * p[1] - q[1] * p[3]),
                        q[0] * p[3] + p[0] * q[3] + (q[1] * p[2] - q[2] * p[1])]
                done[b] = True; span = True; seq.append(j)
            if not done[a] and done[b]:
                p = Q[b]
                na = -q[0]
                Q[a] = [na * p[0] - (q[1] * p[1] + q[2] * p[2] + q[3] * p[3]),
                        na * p[1] + p[0] * q[1] + (q[2] * p[3] - q[3] * p[2]),
                        na * p[2] + p[0] * q[2] + (q[3] * p[1] - q[1] * p[3]),
                        na * p[3] + p[0] * q[3] + (q[1] * p[2] - q[2] * p[1])]
                done[a] = True; span = True; seq.append(j)
        if not span and done.sum() < N:
            raise ValueError("Relative rotations DO NOT SPAN all the nodes in the VIEW GRAPH")
    return Q, passes, seq


def amatrix(I, N):
    """BoxMedianSO3Graph.m:116-121: sparse m x (N-1), -1 at I(1,:), +1 at I(2,:), node 1 dropped."""
    m = I.shape[1]
    rows = np.repeat(np.arange(m), 2); cols = I.T.reshape(-1) - 1; vals = np.tile([-1.0, 1.0], m)
    k = cols != 0
    return scipy.sparse.csr_matrix((vals[k], (rows[k], cols[k] - 1)), shape=(m, N - 1))


def l1decode_pd(x0, A, y, pdtol=1e-3, pdmaxiter=50, trace=None):
    """BoxMedianSO3Graph.m:245-360 (l1-magic); A sparse.  trace (dict, optional) gets 'steps', 'ill', 'stuck' counts."""
    tr = trace if trace is not None else {}
    N = x0.shape[0]; M = y.shape[0]
    alpha, beta, mu = 0.01, 0.5, 10
    x = x0.copy(); Ax = A @ x
    with np.errstate(all="ignore"):
        u = 0.95 * np.abs(y - Ax) + 0.10 * np.max(np.abs(y - Ax))
        fu1 = Ax - y - u; fu2 = -Ax + y - u
        lamu1 = -1 / fu1; lamu2 = -1 / fu2
        Atv = A.T @ (lamu1 - lamu2)
        sdg = -(fu1 @ lamu1 + fu2 @ lamu2)
        tau = mu * 2 * M / sdg
        rcent = np.concatenate([-lamu1 * fu1, -lamu2 * fu2]) - (1 / tau)
        rdual = np.concatenate([Atv, 1 + (-lamu1 - lamu2)])
        resnorm = np.linalg.norm(np.concatenate([rdual, rcent]))
    pditer = 0
    done = (sdg < pdtol) | (pditer >= pdmaxiter)
    As = scipy.sparse.csr_matrix(A)
    while not done:
        pditer += 1
        with np.errstate(all="ignore"):
            w2 = -1 - 1 / tau * (1 / fu1 + 1 / fu2)
            sig1 = -lamu1 / fu1 - lamu2 / fu2
            sig2 = lamu1 / fu1 - lamu2 / fu2
            sigx = sig1 - sig2 ** 2 / sig1
            w1 = -1 / tau * (A.T @ (-1 / fu1 + 1 / fu2))
            w1p = w1 - A.T @ ((sig2 / sig1) * w2)
            H11p = (As.T @ scipy.sparse.diags(sigx) @ As).toarray()      # AtDiagA (:206-209), dense
        if not np.all(np.isfinite(H11p)):
            hcond = np.nan                                         # MATLAB: rcond of a NaN matrix is NaN; NaN < 1e-14 is false
            dx = np.full(N, np.nan)
        else:
            lu, piv = scipy.linalg.lu_factor(H11p, check_finite=False)
            anorm = np.abs(H11p).sum(axis=0).max()
            hcond = scipy.linalg.lapack.dgecon(lu, anorm, norm="1")[0]
            dx = scipy.linalg.lu_solve((lu, piv), w1p, check_finite=False)
        tr["steps"] = tr.get("steps", 0) + 1
        if hcond < 1e-14:
            tr["ill"] = tr.get("ill", 0) + 1
            tr["steps"] -= 1
            return x
        with np.errstate(all="ignore"):
            Adx = A @ dx
            du = (w2 - sig2 * Adx) / sig1
            dlamu1 = -(lamu1 / fu1) * (Adx - du) - lamu1 - (1 / tau) * 1 / fu1
            dlamu2 = (lamu2 / fu2) * (Adx + du) - lamu2 - (1 / tau) * 1 / fu2
            Atdv = A.T @ (dlamu1 - dlamu2)
            cand = np.concatenate([[1.0], (-lamu1 / dlamu1)[dlamu1 < 0], (-lamu2 / dlamu2)[dlamu2 < 0]])
            s = np.nanmin(cand)                                    # MATLAB's min ignores NaN
            d1 = Adx - du; d2 = -Adx - du
            cand = np.concatenate([[s], (-fu1 / d1)[d1 > 0], (-fu2 / d2)[d2 > 0]])
            s = 0.99 * np.nanmin(cand)
        backiter = 0
        while True:
            with np.errstate(all="ignore"):
                xp = x + s * dx; up = u + s * du
                Axp = Ax + s * Adx; Atvp = Atv + s * Atdv
                lamu1p = lamu1 + s * dlamu1; lamu2p = lamu2 + s * dlamu2
                fu1p = Axp - y - up; fu2p = -Axp + y - up
                rdp = np.concatenate([Atvp, 1 + (-lamu1p - lamu2p)])
                rcp = np.concatenate([-lamu1p * fu1p, -lamu2p * fu2p]) - (1 / tau)
                suffdec = np.linalg.norm(np.concatenate([rdp, rcp])) <= (1 - alpha * s) * resnorm
            s = beta * s
            backiter += 1
            if backiter > 32:
                tr["stuck"] = tr.get("stuck", 0) + 1
                return x
            if suffdec:
                break
        x = xp; u = up; Ax = Axp; Atv = Atvp; lamu1 = lamu1p; lamu2 = lamu2p; fu1 = fu1p; fu2 = fu2p
        with np.errstate(all="ignore"):
            sdg = -(fu1 @ lamu1 + fu2 @ lamu2)
            tau = mu * 2 * M / sdg
            rcent = np.concatenate([-lamu1 * fu1, -lamu2 * fu2]) - (1 / tau)
            resnorm = np.linalg.norm(np.concatenate([rdp, rcent]))
        done = (sdg < pdtol) | (pditer >= pdmaxiter)
    return x


def edge_log(I, Q, QQ):
    """BoxMedianSO3Graph.m:143-160 = RobustMeanSO3Graph.m:134-159: B (m x 3), NaN -> 0."""
    i = I[0] - 1; j = I[1] - 1
    w = qmul(QQ, Q[i])
    Qj = Q[j]
    w = np.concatenate([(-Qj[:, 0:1] * w[:, 0:1] - np.sum(Qj[:, 1:4] * w[:, 1:4], axis=1, keepdims=True)),
                        -Qj[:, 0:1] * w[:, 1:4] + w[:, 0:1] * Qj[:, 1:4] +
                        np.stack([Qj[:, 2] * w[:, 3] - Qj[:, 3] * w[:, 2], Qj[:, 3] * w[:, 1] - Qj[:, 1] * w[:, 3], Qj[:, 1] * w[:, 2] - Qj[:, 2] * w[:, 1]], axis=1)], axis=1)
    s2 = np.sqrt(np.sum(w[:, 1:4] ** 2, axis=1))
    w[:, 0] = 2 * np.arctan2(s2, w[:, 0])
    w[w[:, 0] < -np.pi, 0] += 2 * np.pi
    w[w[:, 0] >= np.pi, 0] -= 2 * np.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        B = w[:, 1:4] * (w[:, 0] / s2)[:, None]
    B[np.isnan(B)] = 0
    return B


def exp_update(Q, X):
    """W(2:end,2:4) = X; exp map with NaN -> 0; Q <- Q * W (BoxMedianSO3Graph.m:175-185)."""
    N = Q.shape[0]
    W = np.zeros((N, 4)); W[0] = [1, 0, 0, 0]; W[1:, 1:4] = X
    theta = np.sqrt(np.sum(W[:, 1:4] ** 2, axis=1))
    W[:, 0] = np.cos(theta / 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        W[:, 1:4] = W[:, 1:4] * (np.sin(theta / 2) / theta)[:, None]
    W[np.isnan(W)] = 0
    return qmul(Q, W)


def box_median(RR, I, Rinit=None, maxIters=100, trace=None):
    """BoxMedianSO3Graph.m:51-203 for the matrix form."""
    tr = trace if trace is not None else {}
    N = int(I.max())
    QQ = R2Q(RR)
    if Rinit is not None:
        Q = R2Q(Rinit)
    else:
        Q, tr["tree_passes"], tr["tree_seq"] = tree_start(I, QQ, N)
    tr["Q0"] = Q.copy()
    A = amatrix(I, N)
    changeThreshold = .001; score = np.inf; Iteration = 0; L1Step = 2
    scores = []
    while ((score >= changeThreshold) or (L1Step < 2)) and (Iteration < maxIters):
        if score < changeThreshold:
            L1Step = L1Step * 4; changeThreshold = changeThreshold / 100
        B = edge_log(I, Q, QQ)
        X = np.zeros((N - 1, 3))
        for c in range(3):
            X[:, c] = l1decode_pd(X[:, c], A, B[:, c], EPS, L1Step, trace=tr)
        score = np.max(np.sqrt(np.sum(X * X, axis=1)))
        Q = exp_update(Q, X)
        Iteration += 1
        scores.append(score)
    tr["l1_iters"] = Iteration; tr["l1_scores"] = scores
    R = np.stack([np.real(q2R(Q[v])) for v in range(N)], axis=2)
    return R


def robust_mean(RR, I, SIGMA, Rinit, maxIters=100, mode="GM", trace=None):
    """RobustMeanSO3Graph.m (mode 'GM') / L12.m (mode 'L12'), given Rinit; normal equations, dense solve."""
    tr = trace if trace is not None else {}
    SIGMA = SIGMA * np.pi / 180
    N = int(I.max())
    QQ = R2Q(RR)
    Q = R2Q(Rinit)
    A = amatrix(I, N)
    m = I.shape[1]
    Weights = np.ones(m)
    score = np.inf; Iteration = 0
    scores = []
    while score > 1e-3 and Iteration < maxIters:
        B = edge_log(I, Q, QQ)
        W2 = scipy.sparse.diags(Weights * Weights)
        H = (A.T @ W2 @ A).toarray()
        rhs = A.T @ (W2 @ B)
        X = scipy.linalg.cho_solve(scipy.linalg.cho_factor(H), rhs)
        E = A @ X - B
        if mode == "GM":
            Weights = SIGMA / (np.sum(E ** 2, axis=1) + SIGMA ** 2)
        else:
            residualE = np.sqrt(np.sum(E ** 2, axis=1))
            with np.errstate(divide="ignore"):
                Weights = 1 / (residualE ** 0.75)
            Weights[Weights > 1e4] = 1e4
        score = np.sum(np.sqrt(np.sum(X * X, axis=1))) / N
        Q = exp_update(Q, X)
        Iteration += 1
        scores.append(score)
    tr["irls_iters"] = Iteration; tr["irls_scores"] = scores
    return np.stack([q2R(Q[v]) for v in range(N)], axis=2)


def irls_oracle(RijMat, Ind, mode="GM", Rinit=None, SIGMA=5, MaxIterations=(10, 100)):
    """R = IRLS_GM / IRLS_L12(RijMat, Ind, ...) -> (R 3x3xN with NaN outside the component, R_l1 likewise, trace dict)."""
    Ind = np.asarray(Ind, dtype=np.int64)
    RR = np.transpose(np.asarray(RijMat, dtype=np.float64), (1, 0, 2))           # :52
    I = Ind.T                                                                      # :53
    N = int(I.max())
    nodes, emask = largest_component(Ind, N)                                       # :65-67
    RR, warned = project(RR)                                                       # :82-93
    newid = np.full(N, -1); newid[nodes] = np.arange(nodes.size)
    Ic = newid[I[:, emask] - 1] + 1
    RRc = RR[:, :, emask]
    tr = dict(warned=warned, comp_nodes=int(nodes.size), comp_edges=int(emask.sum()))
    Ri = None if Rinit is None else np.asarray(Rinit, dtype=np.float64)[:, :, nodes]
    R1c = box_median(RRc, Ic, Ri, MaxIterations[0], trace=tr)
    Rc = robust_mean(RRc, Ic, SIGMA, R1c, MaxIterations[1], mode=mode, trace=tr)
    R = np.full((3, 3, N), np.nan); R1 = np.full((3, 3, N), np.nan)
    R[:, :, nodes] = Rc; R1[:, :, nodes] = R1c
    for k in ("steps", "ill", "stuck"):
        tr.setdefault(k, 0)
    return R, R1, tr

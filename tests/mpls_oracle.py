"""ORACLE -- test infrastructure only.  NumPy restatement of the reference's ``Algorithms/MPLS.m:31-257`` (small n).

PARITY UNPINNED by the reference (no fixtures; MATLAB cannot run here).  ``datasample`` is replaced by the keyed rule shared with
the product (oracle/cemp_oracle.py); ``minspantree`` by Kruskal over the order (fl(SVec + 1), edge index) with union-find;
``Weighted_LAA`` and ``quantile`` as in oracle/refine_oracle.py (``lstsq``, ``method="hazen"``).  Unlike oracle/cemp_oracle.py this
keeps the whole ``S0Mat`` -- including the columns of the edges without a 3-cycle, whose cycle product is the zero matrix
(MPLS.m:109-130: ``|acos(-1/2)|/pi = 2/3``) -- and the cycles' edge ids, which the MPLS loop re-uses (:223-237)."""
import numpy as np

from oracle.cemp_oracle import _mix64_v
from oracle.desc_pgd_literal import matlab_abs_acos
from oracle.refine_oracle import Build_Amatrix, R2Q, Weighted_LAA, q2R


def padded(v, T):
    """MPLS.m:37-63: a parameter vector shorter than T repeats its last entry."""
    v = list(np.atleast_1d(np.asarray(v, dtype=np.float64)).reshape(-1))
    return v + [v[-1]] * (T - len(v)) if len(v) < T else v


def cemp_stage(Ind, RijMat, max_iter, reweighting, nsample, seed=0):
    """MPLS.m:65-158 -> dict(SVec, S0Mat (nsample x m), Eki, Ejk (edge ids of {k,i}, {j,k}), IndPosbin)."""
    Ind = np.asarray(Ind, dtype=np.int64)
    T = int(max_iter)
    beta_cemp = padded(reweighting, T)
    Ind_i, Ind_j = Ind[:, 0] - 1, Ind[:, 1] - 1
    n = int(Ind.max()); m = Ind.shape[0]
    A = np.zeros((n, n), dtype=bool); A[Ind_i, Ind_j] = True; A |= A.T                   # :70-71
    eid = np.full((n, n), -1, dtype=np.int64); eid[Ind_i, Ind_j] = np.arange(m); eid[Ind_j, Ind_i] = np.arange(m)     # |IndMat| - 1
    R = np.ascontiguousarray(np.transpose(np.asarray(RijMat, dtype=np.float64), (2, 0, 1)))
    common = A[Ind_i] & A[Ind_j]                                                          # :78
    codeg = common.sum(axis=1)
    IndPosbin = codeg > 0                                                                 # :79-87
    S0Mat = np.zeros((nsample, m)); Eki = np.zeros((nsample, m), dtype=np.int64); Ejk = np.zeros((nsample, m), dtype=np.int64)
    Rc = np.zeros((nsample, m, 3, 3))                                                     # Rki0 / Rjk0 stay zero without cycles (:109-110)
    pos = np.flatnonzero(IndPosbin)
    if pos.size:
        tt = np.arange(nsample, dtype=np.uint64)[:, None]
        l = pos.astype(np.uint64)[None, :]
        with np.errstate(over="ignore"):
            key = _mix64_v(_mix64_v(np.uint64(seed) ^ ((l + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))) ^ ((tt + np.uint64(1)) * np.uint64(0xD1B54A32D192ED03)))
        idx = (key % codeg[pos].astype(np.uint64)[None, :]).astype(np.int64)               # :93 with the keyed stand-in
        k = np.zeros((nsample, pos.size), dtype=np.int64)
        for c, e in enumerate(pos):
            k[:, c] = np.flatnonzero(common[e])[idx[:, c]]
        i, j = Ind_i[pos][None, :], Ind_j[pos][None, :]
        ejk, eki = eid[j, k], eid[i, k]
        Rjk = np.where((j < k)[..., None, None], R[ejk], np.transpose(R[ejk], (0, 1, 3, 2)))     # RijMat4d(:,:,j,k)  (:113)
        Rki = np.where((k < i)[..., None, None], R[eki], np.transpose(R[eki], (0, 1, 3, 2)))     # RijMat4d(:,:,k,i)  (:112)
        Rc[:, pos] = np.matmul(np.matmul(R[pos][None], Rjk), Rki)                          # :123-128
        Eki[:, pos] = eki; Ejk[:, pos] = ejk
    tr = Rc[..., 0, 0] + Rc[..., 1, 1] + Rc[..., 2, 2]                                    # :129
    S0Mat = matlab_abs_acos(((tr - 1) / 2).reshape(-1)).reshape(tr.shape) / np.pi        # :130
    SVec = S0Mat.mean(axis=0)                                                             # :131
    SVec[~IndPosbin] = 1                                                                  # :132
    for it in range(T):                                                                   # :136-157
        Wm = np.exp(-beta_cemp[it] * (np.where(IndPosbin, SVec[Eki], 0.0) + np.where(IndPosbin, SVec[Ejk], 0.0)))
        Wm = Wm / Wm.sum(axis=0)
        SVec = (Wm * S0Mat).sum(axis=0)
        SVec[~IndPosbin] = 1
    return dict(SVec=SVec, S0Mat=S0Mat, Eki=Eki, Ejk=Ejk, IndPosbin=IndPosbin)


def h_step(st, ResVec, beta):
    """MPLS.m:223-237: HVec from the residuals through CEMP's samples (no reset of the edges without cycles, :239)."""
    P = st["IndPosbin"]
    Ski = np.where(P, ResVec[st["Eki"]], 0.0); Sjk = np.where(P, ResVec[st["Ejk"]], 0.0)
    Wm = np.exp(-beta * (Ski + Sjk))
    Wm = Wm / Wm.sum(axis=0)
    return (Wm * st["S0Mat"]).sum(axis=0)


def kruskal(Ind, SVec):
    """minspantree of MPLS.m:162-168 with the order (fl(SVec + 1), edge index): ascending 0-based edge ids of the tree, or None
    if the graph is not connected."""
    Ind = np.asarray(Ind, dtype=np.int64)
    n = int(Ind.max()); m = Ind.shape[0]
    key = np.asarray(SVec, dtype=np.float64) + 1.0
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    tree = []
    for e in np.lexsort((np.arange(m), key)):
        a, b = find(int(Ind[e, 0]) - 1), find(int(Ind[e, 1]) - 1)
        if a != b:
            parent[max(a, b)] = min(a, b)
            tree.append(int(e))
    return np.array(sorted(tree), dtype=np.int64) if len(tree) == n - 1 else None


def propagate(Ind, RijMat, tree):
    """MPLS.m:171-193: R_1 = I, breadth first from node 1; R_leaf = R_e R_root if the leaf is e's smaller endpoint, R_e' R_root else."""
    Ind = np.asarray(Ind, dtype=np.int64)
    n = int(Ind.max())
    nb = [[] for _ in range(n)]
    for e in tree:
        i, j = int(Ind[e, 0]) - 1, int(Ind[e, 1]) - 1
        nb[i].append((j, e)); nb[j].append((i, e))
    R = np.zeros((3, 3, n)); R[:, :, 0] = np.eye(3)
    added = np.zeros(n, dtype=bool); added[0] = True
    queue = [0]
    for root in queue:
        for leaf, e in nb[root]:
            if added[leaf]:
                continue
            Re = RijMat[:, :, e] if leaf == int(Ind[e, 0]) - 1 else RijMat[:, :, e].T
            R[:, :, leaf] = Re @ R[:, :, root]
            added[leaf] = True; queue.append(leaf)
    return R


def mpls_oracle(Ind, RijMat, CEMP_parameters, MPLS_parameters, seed=0, svec_for_tree=None):
    """MPLS.m:31-257 -> dict(R_est, R_init, SVec, iters, score, tree, scores: every step's score).  ``svec_for_tree``: build the tree from this SVec (the
    device's) instead of the oracle's own -- two keys within round-off of each other could otherwise pick different trees."""
    Ind = np.asarray(Ind, dtype=np.int64)
    RijMat = np.asarray(RijMat, dtype=np.float64)
    n = int(Ind.max())
    st = cemp_stage(Ind, RijMat, CEMP_parameters["max_iter"], CEMP_parameters["reweighting"], CEMP_parameters["nsample"], seed)
    maxIters = int(MPLS_parameters["max_iter"])
    beta = padded(MPLS_parameters["reweighting"], maxIters)
    tau = padded(MPLS_parameters["thresholding"], maxIters)
    alpha = padded(MPLS_parameters["cycle_info_ratio"], maxIters)
    SVec = st["SVec"]
    tree = kruskal(Ind, SVec if svec_for_tree is None else svec_for_tree)
    R_init = propagate(Ind, RijMat, tree)
    Ind_T = Ind.T
    Amatrix = Build_Amatrix(Ind_T)                                                        # :204
    Q = R2Q(R_init); QQ = R2Q(np.transpose(RijMat, (1, 0, 2)))                            # :200-206
    score = np.inf; Iteration = 1
    Weights = 1.0 / (SVec ** 0.75)                                                        # :210
    Weights[Weights > 1e4] = 1e4                                                          # :211-213
    scores = []
    while score > MPLS_parameters["stop_threshold"] and Iteration < maxIters:            # :218
        Q, W, B, score = Weighted_LAA(Ind_T, Q, QQ, Amatrix, Weights)                     # :220
        scores.append(float(score))
        E = Amatrix @ W[1:, 1:4] - B                                                      # :221
        ResVec = np.sqrt(np.sum(E ** 2, axis=1)) / np.pi                                  # :222
        HVec = h_step(st, ResVec, beta[Iteration - 1])                                    # :223-237
        RHVec = (1 - alpha[Iteration - 1]) * ResVec + alpha[Iteration - 1] * HVec         # :240
        Weights = 1.0 / (RHVec ** 0.75)                                                   # :241
        thresh = np.quantile(RHVec, tau[Iteration - 1], method="hazen")                   # :243
        Weights[Weights > 1e4] = 1e4
        Weights[RHVec > thresh] = 1e-4
        Iteration += 1
    R_est = np.zeros((3, 3, n))
    for i in range(n):
        R_est[:, :, i] = q2R(Q[i])                                                        # :251-254
    return dict(R_est=R_est, R_init=R_init, SVec=SVec, iters=Iteration - 1, score=score, tree=tree, state=st, scores=scores)

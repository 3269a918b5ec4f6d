"""ORACLE -- test infrastructure only.  NumPy / SciPy restatement of the reference's ``Algorithms/linprog_sij.m`` (small n).

PARITY UNPINNED by the reference (no fixtures; MATLAB cannot run here).  ``datasample(..., 'Replace', true)`` (:68) is replaced by
the keyed rule shared with the product: the t-th sample of edge l is ``CoInd[sample_key(seed, l, t) mod codeg]`` (CoInd ascending).
One deliberate departure, as in the product: :84-85 index ``Ind_i(l)`` / ``Ind_j(l)`` with l running over the edges with cycles,
which is the wrong edge as soon as some edge has no cycle; the edge's own endpoints are used here (:66 and CEMP.m do the same).

The LP (:107-139): variables = the edges with cycles in ascending edge order; per variable l and sample t with d = S0Mat(t, l),
a = edge {i,k}, b = edge {j,k}: rows  s_l - s_a - s_b <= d  and  -s_l - s_a - s_b <= -d  (in this order, rows 2 (l nsample + t) and
the next); 0 <= s <= 1; cost all ones.  The LP optimum is not unique: solutions are compared through ``certificates``."""
import numpy as np
import scipy.optimize
import scipy.sparse as sp

from oracle.cemp_oracle import _mix64_v
from oracle.desc_pgd_literal import matlab_abs_acos, matlab_median
from oracle.refine_oracle import desc_refine_oracle
from oracle.spectral_oracle import _blk, _project


def rule_nsample(codeg_pos):
    """linprog_sij.m:43 (the rule of DESC_PGD.m:43): max(ceil(median(codeg of the edges with cycles) / 4), 30)."""
    if len(codeg_pos) == 0:
        return 30
    return int(max(np.ceil(matlab_median(np.asarray(codeg_pos, dtype=np.float64)) / 4.0), 30))


def lp_arrays(Ind, RijMat, seed, nsample=None):
    """-> (own, va, vb (m_pos nsample each: the three columns of cycle c = l nsample + t, variable indices), d (m_pos x nsample: S0Mat(t, l) at
    [l][t]), pos (0-based edge ids with cycles, ascending), k (m_pos x nsample, 1-based), nsample).  ``Ind`` must be sorted by (i, j)."""
    Ind = np.asarray(Ind, dtype=np.int64)
    Ind_i, Ind_j = Ind[:, 0] - 1, Ind[:, 1] - 1
    n = int(Ind.max()); m = Ind.shape[0]
    A = np.zeros((n, n), dtype=bool); A[Ind_i, Ind_j] = True; A |= A.T                      # :21-23
    eid = np.full((n, n), -1, dtype=np.int64); eid[Ind_i, Ind_j] = np.arange(m); eid[Ind_j, Ind_i] = np.arange(m)
    R = np.ascontiguousarray(np.transpose(np.asarray(RijMat, dtype=np.float64), (2, 0, 1)))
    common = A[Ind_i] & A[Ind_j]                                                            # :29
    codeg = common.sum(axis=1)
    pos = np.flatnonzero(codeg > 0)                                                         # :30-41
    if nsample is None:
        nsample = rule_nsample(codeg[pos])                                                  # :43
    mp = pos.size
    var = np.full(m, -1, dtype=np.int64); var[pos] = np.arange(mp)
    tt = np.arange(nsample, dtype=np.uint64)[None, :]
    l = pos.astype(np.uint64)[:, None]
    with np.errstate(over="ignore"):
        key = _mix64_v(_mix64_v(np.uint64(seed) ^ ((l + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))) ^ ((tt + np.uint64(1)) * np.uint64(0xD1B54A32D192ED03)))
    idx = (key % np.maximum(codeg[pos], 1).astype(np.uint64)[:, None]).astype(np.int64)      # :68 with the keyed stand-in
    k = np.zeros((mp, nsample), dtype=np.int64)
    for c, e in enumerate(pos):
        k[c] = np.flatnonzero(common[e])[idx[c]]
    i, j = Ind_i[pos][:, None], Ind_j[pos][:, None]
    eki, ejk = eid[i, k], eid[j, k]                                                         # the edge's own endpoints (not :84-85)
    Rjk = np.where((j < k)[..., None, None], R[ejk], np.transpose(R[ejk], (0, 1, 3, 2)))
    Rki = np.where((k < i)[..., None, None], R[eki], np.transpose(R[eki], (0, 1, 3, 2)))
    Rc = np.matmul(np.matmul(R[pos][:, None], Rjk), Rki)                                    # :88-100
    tr = Rc[..., 0, 0] + Rc[..., 1, 1] + Rc[..., 2, 2]
    d = matlab_abs_acos(((tr - 1) / 2).reshape(-1)).reshape(tr.shape) / np.pi               # S0Mat(t, l), here [l][t]  (:101)
    own = np.repeat(np.arange(mp), nsample); va = var[eki.reshape(-1)]; vb = var[ejk.reshape(-1)]
    assert (va >= 0).all() and (vb >= 0).all()          # the edges ik, jk of a triangle lie on that triangle
    return own, va, vb, d, pos, k + 1, nsample


def build_lp(Ind, RijMat, seed, nsample=None):
    """-> (K (2 m_pos nsample x m_pos, CSR), b, pos (0-based edge ids with cycles, ascending), k (m_pos x nsample, 1-based), nsample).
    ``Ind`` must be sorted by (i, j)."""
    own, va, vb, d, pos, k, nsample = lp_arrays(Ind, RijMat, seed, nsample)
    mp = pos.size
    nc = mp * nsample
    rows = np.arange(nc)
    r = np.concatenate([2 * rows, 2 * rows, 2 * rows, 2 * rows + 1, 2 * rows + 1, 2 * rows + 1])
    c = np.concatenate([own, va, vb, own, va, vb])
    v = np.concatenate([np.ones(nc), -np.ones(nc), -np.ones(nc), -np.ones(nc), -np.ones(nc), -np.ones(nc)])
    K = sp.csr_matrix((v, (r, c)), shape=(2 * nc, mp))                                       # :107-131
    b = np.empty(2 * nc); b[0::2] = d.reshape(-1); b[1::2] = -d.reshape(-1)
    return K, b, pos, k, nsample


def solve_highs(K, b):
    """-> (f*, x*, y* >= 0): the LP by HiGHS's interior point (the dual simplex needs minutes from n = 100 on)."""
    res = scipy.optimize.linprog(np.ones(K.shape[1]), A_ub=K, b_ub=b, bounds=(0, 1), method="highs-ipm")
    assert res.status == 0, res.message
    return float(res.fun), np.asarray(res.x), -np.asarray(res.ineqlin.marginals)


def step_sizes(K):
    """The documented diagonal steps (Pock-Chambolle, alpha = 1): tau_l = 1 / sum_r |K_rl|, sigma_r = 1 / sum_l |K_rl| (= 1/3)."""
    Ka = abs(K)
    return 1.0 / np.asarray(Ka.sum(axis=0)).reshape(-1), 1.0 / np.asarray(Ka.sum(axis=1)).reshape(-1)


def pdhg_plain(K, b, tau, sigma, N):
    """N steps of x+ = clip(x - tau (1 + K'y), 0, 1), y+ = max(y + sigma (K (2 x+ - x) - b), 0) from x = 0, y = 0."""
    x = np.zeros(K.shape[1]); y = np.zeros(K.shape[0])
    KT = K.T.tocsr()
    for _ in range(N):
        xn = np.clip(x - tau * (1.0 + KT @ y), 0.0, 1.0)
        y = np.maximum(y + sigma * (K @ (2.0 * xn - x) - b), 0.0)
        x = xn
    return x, y


def _margin(a, b):
    """Relative distance of the two sides of a comparison (inf against an infinite side, 0 for 0 against 0)."""
    a, b = float(a), float(b)
    if np.isinf(a) or np.isinf(b):
        return np.inf
    big = max(abs(a), abs(b))
    return abs(a - b) / big if big > 0 else 0.0


def pdhg_loop(own, va, vb, d, m_pos, nsample, max_iter, tol, check_every=64, restart=True, dtype=np.float64):
    """The loop of desc_amd/csrc/lp.hip (its head comment), matrix-free: cycle c = l nsample + t has the columns own[c] = l, va[c], vb[c] and
    the rows  x_l - x_a - x_b <= d_c  (dual y[c, 0]) and  -x_l - x_a - x_b <= -d_c  (dual y[c, 1]).  Every number is kept in ``dtype``.
    -> dict: x (m_pos), y (m_pos x nsample x 2), iters, restarts, converged, rec = (viol, P, D) of the returned point, and log, one entry
    per check: it, avg (the average was the candidate), fired (None, "0.2", "0.8+grew", "period": the restart condition), margins
    (name -> relative margin of every comparison that was evaluated on the way to what the check did: "avg" e_avg against e_cur, "0.2" and
    "0.8" e against that part of e_restart, "grew" e against e_prev, "period" cnt against 0.36 it, "stop" the stopping test: the closer of
    its two comparisons when it passed, the farther of the failed ones when it did not)."""
    T = dtype
    mp, ns = int(m_pos), int(nsample)
    nc = mp * ns
    own, va, vb = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (own, va, vb))
    d = np.asarray(d).reshape(-1).astype(T)
    assert own.size == va.size == vb.size == d.size == nc
    one, zero = T(1), T(0)
    inc = np.bincount(va, minlength=mp) + np.bincount(vb, minlength=mp)
    tau = one / (T(2) * T(ns) + T(2) * inc.astype(T))
    sigma = one / T(3)
    checks = bool(restart) or tol > 0
    tolT = T(tol)

    def reduced_cost(y1, y2):                                   # 1 + K'y
        r = np.zeros(mp, dtype=T)
        np.add.at(r, own, y1 - y2)
        z = y1 + y2
        np.add.at(r, va, -z); np.add.at(r, vb, -z)
        return one + r

    def record(x, y1, y2):                                      # (viol, P, D)
        s = x[va] + x[vb]; xl = x[own]
        viol = max(np.maximum((xl - s) - d, (-xl - s) + d).max(), zero) if nc else zero
        return viol, x.sum(dtype=T), -(d * (y1 - y2)).sum(dtype=T) + np.minimum(reduced_cost(y1, y2), zero).sum(dtype=T)

    def error_of(r):
        return max(r[0], abs(r[1] - r[2]) / (one + abs(r[1]) + abs(r[2])))

    x = np.zeros(mp, dtype=T); y1 = np.zeros(nc, dtype=T); y2 = np.zeros(nc, dtype=T)
    xs, y1s, y2s = x.copy(), y1.copy(), y2.copy()
    e_restart = e_prev = T(np.inf)
    cnt = it = restarts = 0
    converged = False
    fin = None
    log = []
    while it < max_iter:
        it += 1
        xn = np.clip(x - tau * reduced_cost(y1, y2), zero, one)
        xbar = T(2) * xn - x
        x = xn
        s = xbar[va] + xbar[vb]; xl = xbar[own]
        y1 = np.maximum(y1 + sigma * ((xl - s) - d), zero)
        y2 = np.maximum(y2 + sigma * ((-xl - s) + d), zero)
        cnt += 1
        if restart:
            xs = xs + x; y1s = y1s + y1; y2s = y2s + y2
        if not checks or (it % check_every != 0 and it != max_iter):
            continue
        margins = {}
        cand = (x, y1, y2); rec = record(*cand)
        use_avg = False
        if restart:
            avg = (xs / T(cnt), y1s / T(cnt), y2s / T(cnt)); rec_avg = record(*avg)
            use_avg = bool(error_of(rec_avg) <= error_of(rec))
            margins["avg"] = _margin(error_of(rec_avg), error_of(rec))
            if use_avg:
                cand, rec = avg, rec_avg
        e = error_of(rec)
        fin = (cand, rec)
        entry = dict(it=it, avg=use_avg, fired=None, margins=margins)
        log.append(entry)
        if tol > 0:
            P, D = rec[1], rec[2]
            two = [(rec[0], tolT), (P - D, tolT * (one + abs(P) + abs(D)))]
            ok = [bool(a <= b) for a, b in two]
            m2 = [_margin(a, b) for a, b in two]
            margins["stop"] = min(m2) if all(ok) else max(mm for mm, o in zip(m2, ok) if not o)
            if all(ok):
                converged = True
                break
        if not restart or it == max_iter:
            continue
        margins["0.2"] = _margin(e, T(0.2) * e_restart)
        if e <= T(0.2) * e_restart:
            entry["fired"] = "0.2"
        else:
            margins["0.8"] = _margin(e, T(0.8) * e_restart)
            if e <= T(0.8) * e_restart:
                margins["grew"] = _margin(e, e_prev)
                if e > e_prev:
                    entry["fired"] = "0.8+grew"
            if entry["fired"] is None:
                margins["period"] = _margin(T(cnt), T(0.36) * T(it))
                if T(cnt) >= T(0.36) * T(it):
                    entry["fired"] = "period"
        if entry["fired"] is not None:
            if use_avg:
                x, y1, y2 = cand
            xs = np.zeros(mp, dtype=T); y1s = np.zeros(nc, dtype=T); y2s = np.zeros(nc, dtype=T)
            e_restart = e; e_prev = T(np.inf); cnt = 0; restarts += 1
        else:
            e_prev = e
    if fin is None:
        fin = ((x, y1, y2), record(x, y1, y2))
    (xf, y1f, y2f), rec = fin
    return dict(x=xf, y=np.stack([y1f, y2f], axis=1).reshape(mp, ns, 2), iters=it, restarts=restarts, converged=converged, rec=rec, log=log)


def same_decisions(a, b):
    """Two pdhg_loop results took the same way through the loop."""
    key = lambda r: (r["iters"], r["restarts"], r["converged"], [(g["it"], g["avg"], g["fired"]) for g in r["log"]])      # noqa: E731
    return key(a) == key(b)


def certificates(K, b, x, y):
    """-> (viol, P, D): viol = max_r max((Kx - b)_r, 0), P = sum x, D = -b'y + sum_l min(0, 1 + (K'y)_l) (<= f* for every y >= 0)."""
    viol = float(np.maximum(K @ x - b, 0.0).max()) if K.shape[0] else 0.0
    rc = 1.0 + K.T @ y
    return viol, float(x.sum()), float(-(b @ y) + np.minimum(rc, 0.0).sum())


def weighted_spectral(Ind, RijMat, w):
    """linprog_sij.m:154-174: the row-normalised weighted connection matrix, its top three eigenvectors, projection (as GCW.m:9-36)."""
    Ind = np.asarray(Ind, dtype=np.int64)
    n = int(Ind.max())
    B = _blk(Ind, RijMat, n)
    W = np.zeros((n, n)); W[Ind[:, 0] - 1, Ind[:, 1] - 1] = w; W = W + W.T
    W = W / W.sum(axis=1)[:, None]
    import scipy.linalg
    lam, vec = scipy.linalg.eig(B * np.kron(W, np.ones((3, 3))))
    V = np.real(vec[:, np.argsort(-lam.real)[:3]])
    return _project(V / np.linalg.norm(V, axis=0), n)


def tail(Ind, RijMat, S_vec):
    """linprog_sij.m:154-351 -> (R_gcw, Rest): the weighted spectral step with exp(-5 S), then DESC.m:265-313 with maxIters = 200."""
    R_gcw = weighted_spectral(Ind, RijMat, np.exp(-5.0 * np.asarray(S_vec)))
    Rest, iters, score = desc_refine_oracle(Ind, RijMat, np.asarray(S_vec), R_gcw, maxIters=200)
    return R_gcw, Rest

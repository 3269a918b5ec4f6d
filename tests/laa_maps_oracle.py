"""ORACLE -- test infrastructure only.  Two references for the operations of the Lie-algebraic averaging core
(desc_amd/csrc/laa.hip, laa.h, and k_irls_project / k_irls_weights / k_l1_node_update of irls.hip).  The projection is the exception:
its Jacobi SVD is not restated step by step, so (a) covers only its determinant (and the statuses through NumPy's singular values),
and P is compared with (b) alone.

  (a) ``*_a``: a float64 NumPy restatement with the operand order and bracketing of the kernel text (laa.h: "operand order and
      bracketing are part of the interface"; the library is built with -ffp-contract=off).  + - * / and sqrt round correctly on both
      sides, so these are bit-exact models of everything but the libm calls (atan2, sin, cos, pow), where glibc stands in.
  (b) ``*_b``: the same formula in mpmath at 50 digits on the same double inputs (entries are mpf; NaN where the formula is undefined).

Reference text restated (never copied): Utils/R2Q.m:7-14, Utils/q2R.m:1-23, Utils/Weighted_LAA.m:4-51, Utils/Build_Amatrix.m:6-13,
Utils/BoxMedianSO3Graph.m:143-185, Algorithms/DESC.m:276-303, Algorithms/IRLS_GM.m:82-93, MATLAB's quantile (Hazen positions).
Blocks are 9 doubles column-major ((r, c) at r + 3c), quaternions (a, x, y, z), edges 0-based (i < j)."""
import mpmath as mp
import numpy as np

mp.mp.dps = 50
EPS = float(np.finfo(np.float64).eps)
QBINS = 4096
GM, L12 = 0, 1                          # DESC_IRLS_GM / DESC_IRLS_L12 (include/desc_amd.h)


def _quiet(f):
    def g(*a, **k):
        with np.errstate(all="ignore"):
            return f(*a, **k)
    g.__name__, g.__doc__ = f.__name__, f.__doc__
    return g


def bit_equal(x, y):
    """array_equal with NaN positions equal and the signs of zeros and infinities equal."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.shape != y.shape:
        return False
    nx, ny = np.isnan(x), np.isnan(y)
    return bool(np.array_equal(nx, ny) and np.array_equal(x[~nx].view(np.uint64), y[~ny].view(np.uint64)))


def M(a):
    """float array -> object array of exact mpf."""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    for k, v in np.ndenumerate(a):
        out[k] = mp.mpf(float(v))
    return out


def mp_abs_err(x, b):
    """|x - b| per entry as floats (x float array, b mpf array); NaN where b is NaN."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty(x.shape)
    for k, v in np.ndenumerate(x):
        bv = b[k]
        out[k] = np.nan if (mp.isnan(bv) or not np.isfinite(v)) else float(abs(mp.mpf(float(v)) - bv))
    return out


def to_float(b):
    return np.array([float(v) for v in np.asarray(b, dtype=object).reshape(-1)]).reshape(np.shape(b))


# =================================================================================================== quaternion maps
def qmul_a(a, b):
    """laa.h qmul: Hamilton product, rows."""
    a0, a1, a2, a3 = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    b0, b1, b2, b3 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return np.stack([a0 * b0 - ((a1 * b1 + a2 * b2) + a3 * b3),
                     (a0 * b1 + b0 * a1) + (a2 * b3 - a3 * b2),
                     (a0 * b2 + b0 * a2) + (a3 * b1 - a1 * b3),
                     (a0 * b3 + b0 * a3) + (a1 * b2 - a2 * b1)], axis=1)


def qmul_b(a, b):
    return [a[0] * b[0] - (a[1] * b[1] + a[2] * b[2] + a[3] * b[3]),
            a[0] * b[1] + b[0] * a[1] + (a[2] * b[3] - a[3] * b[2]),
            a[0] * b[2] + b[0] * a[2] + (a[3] * b[1] - a[1] * b[3]),
            a[0] * b[3] + b[0] * a[3] + (a[1] * b[2] - a[2] * b[1])]


def _entries(R, transpose):
    R = np.asarray(R).reshape(-1, 9)
    r11, r21, r31, r12, r22, r32, r13, r23, r33 = (R[:, k] for k in range(9))
    if transpose:
        r32, r23, r13, r31, r21, r12 = r23, r32, r31, r13, r12, r21
    return r11, r21, r31, r12, r22, r32, r13, r23, r33


@_quiet
def r2q_a(R, transpose=False):
    """R2Q.m:9-12 as k_r2q writes it.  An exact half-turn gives a = 0 and x/0, 0/0 (R2Q.m:12): inf / NaN carried over."""
    r11, r21, r31, r12, r22, r32, r13, r23, r33 = _entries(np.asarray(R, dtype=np.float64), transpose)
    a = (r11 + r22 + r33 - 1.0) / 2.0
    x = (r32 - r23) / 2.0; y = (r13 - r31) / 2.0; z = (r21 - r12) / 2.0
    a = np.sqrt((a + 1.0) / 2.0)
    return np.stack([a, (x / a) / 2.0, (y / a) / 2.0, (z / a) / 2.0], axis=1)


def r2q_b(R, transpose=False):
    """mpf (count, 4); NaN rows where the square root's argument is negative, a = 0 or an entry is not finite."""
    Rf = np.asarray(R, dtype=np.float64).reshape(-1, 9)
    out = np.empty((Rf.shape[0], 4), dtype=object)
    for t in range(Rf.shape[0]):
        out[t] = [mp.nan] * 4
        if not np.all(np.isfinite(Rf[t])):
            continue
        r11, r21, r31, r12, r22, r32, r13, r23, r33 = (mp.mpf(float(v[0])) for v in _entries(Rf[t:t + 1], transpose))
        arg = ((r11 + r22 + r33 - 1) / 2 + 1) / 2
        if arg <= 0:
            continue
        a = mp.sqrt(arg)
        out[t] = [a, (r32 - r23) / 2 / a / 2, (r13 - r31) / 2 / a / 2, (r21 - r12) / 2 / a / 2]
    return out


@_quiet
def q2r_a(Q):
    """q2R.m as k_q2r writes it: identity when ||a| - 1| <= 1e-12 (q2R.m:4), no renormalisation."""
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 4)
    c2, x, y, z = Q[:, 0], Q[:, 1], Q[:, 2], Q[:, 3]
    s2 = np.sqrt(x * x + y * y + z * z)
    s = 2.0 * s2 * c2; c = 2.0 * c2 * c2 - 1.0; cc = 1.0 - c
    n1 = x / s2; n2 = y / s2; n3 = z / s2
    n12 = n1 * n2 * cc; n23 = n2 * n3 * cc; n31 = n3 * n1 * cc; n1s = n1 * s; n2s = n2 * s; n3s = n3 * s
    R = np.stack([c + n1 * n1 * cc, n12 + n3s, n31 - n2s,
                  n12 - n3s, c + n2 * n2 * cc, n23 + n1s,
                  n31 + n2s, n23 - n1s, c + n3 * n3 * cc], axis=1)
    ident = ~(np.abs(np.abs(c2) - 1.0) > 1e-12)
    R[ident] = np.eye(3).reshape(9)
    return R


def _q2r_b_one(q):
    c2, x, y, z = q
    if mp.isnan(c2) or not (abs(abs(c2) - 1) > mp.mpf(1e-12)):          # a NaN fails the `>` of q2R.m:4 as well: identity
        return [mp.mpf(v) for v in (1, 0, 0, 0, 1, 0, 0, 0, 1)]
    if any(mp.isnan(v) or mp.isinf(v) for v in q):
        return [mp.nan] * 9
    s2 = mp.sqrt(x * x + y * y + z * z)
    if s2 == 0:
        return [mp.nan] * 9
    s = 2 * s2 * c2; c = 2 * c2 * c2 - 1; cc = 1 - c
    n1, n2, n3 = x / s2, y / s2, z / s2
    return [c + n1 * n1 * cc, n1 * n2 * cc + n3 * s, n3 * n1 * cc - n2 * s,
            n1 * n2 * cc - n3 * s, c + n2 * n2 * cc, n2 * n3 * cc + n1 * s,
            n3 * n1 * cc + n2 * s, n2 * n3 * cc - n1 * s, c + n3 * n3 * cc]


def q2r_b(Q):
    """Q: float (n, 4) or mpf (n, 4) -> mpf (n, 9)."""
    Q = np.asarray(Q)
    Qm = Q if Q.dtype == object else M(Q.reshape(-1, 4))
    out = np.empty((Qm.shape[0], 9), dtype=object)
    for t in range(Qm.shape[0]):
        out[t] = _q2r_b_one(list(Qm[t]))
    return out


# =================================================================================================== edge log map
@_quiet
def edge_log_a(ii, jj, Q, QQ, atan_shift=0):
    """k_edge_log (Weighted_LAA.m:9-35).  atan_shift: atan2's result moved by that many ulp (the one libm call of the kernel).
    -> B (m, 3), v (m, 4), the wrapped angle v1 (m)."""
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 4); QQ = np.asarray(QQ, dtype=np.float64).reshape(-1, 4)
    qi, qj = Q[ii], Q[jj]
    w = qmul_a(QQ, qi)
    v = qmul_a(np.stack([-qj[:, 0], qj[:, 1], qj[:, 2], qj[:, 3]], axis=1), w)          # :16-18
    s2 = np.sqrt(v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2] + v[:, 3] * v[:, 3])
    at = np.arctan2(s2, v[:, 0])
    for _ in range(abs(int(atan_shift))):
        at = np.nextafter(at, np.inf if atan_shift > 0 else -np.inf)
    v1 = 2.0 * at
    v1 = np.where(v1 < -np.pi, v1 + 2.0 * np.pi, v1)                                    # :27
    v1 = np.where(v1 >= np.pi, v1 - 2.0 * np.pi, v1)                                    # :28: the sign jump at pi
    f = v1 / s2
    B = v[:, 1:4] * f[:, None]
    B[np.isnan(B)] = 0.0                                                                # :35
    return B, v, v1


def edge_log_b(ii, jj, Q, QQ):
    """mpf B (m, 3) and the edge's exact angle before the wrap (m)."""
    Qm, QQm = M(np.asarray(Q).reshape(-1, 4)), M(np.asarray(QQ).reshape(-1, 4))
    m = len(ii)
    B = np.empty((m, 3), dtype=object); ang = np.empty(m, dtype=object)
    for e in range(m):
        qi, qj, qq = list(Qm[ii[e]]), list(Qm[jj[e]]), list(QQm[e])
        if any(mp.isnan(t) or mp.isinf(t) for t in qi + qj + qq):
            B[e] = [mp.nan] * 3; ang[e] = mp.nan
            continue
        v = qmul_b([-qj[0], qj[1], qj[2], qj[3]], qmul_b(qq, qi))
        s2 = mp.sqrt(v[1] ** 2 + v[2] ** 2 + v[3] ** 2)
        v1 = 2 * mp.atan2(s2, v[0])
        ang[e] = v1
        if v1 >= mp.pi:
            v1 -= 2 * mp.pi
        B[e] = [mp.mpf(0)] * 3 if s2 == 0 else [v[k] * (v1 / s2) for k in (1, 2, 3)]
    return B, ang


# =================================================================================================== normal equations
def csr_rows(n, ii, jj):
    """The library's CSR (build_csr): row v holds its edges with smaller neighbours, then those with larger ones, each ascending --
    for a sorted edge list that is ascending edge order within each half.  -> per node a list of (edge, sign): +1 where v is j."""
    rows = [[] for _ in range(n)]
    lower = [[] for _ in range(n)]
    for e in range(len(ii)):
        rows[ii[e]].append((e, -1.0)); lower[jj[e]].append((e, 1.0))
    return [lower[v] + rows[v] for v in range(n)]


def _tree16(lanes):
    """group16_sum (device_utils.h) as lane 0 receives it: xor 1, xor 2, half-row mirror, row mirror."""
    s = [lanes[k] + lanes[k ^ 1] for k in range(16)]
    s = [s[k] + s[k ^ 2] for k in range(16)]
    s = [s[k] + s[(k & 8) | (7 - (k & 7))] for k in range(16)]
    return s[0] + s[15]


def rhs_a(n, ii, jj, w, B):
    """k_rhs in the kernel's own order: lane l of 16 takes the row's slots l, l + 16, ..., then the butterfly."""
    w = np.asarray(w, dtype=np.float64); B = np.asarray(B, dtype=np.float64).reshape(-1, 3)
    rhs = np.zeros((n, 3)); diag = np.zeros(n)
    with np.errstate(all="ignore"):
        for v, row in enumerate(csr_rows(n, ii, jj)):
            acc = [[np.float64(0.0)] * 16 for _ in range(4)]
            for t, (e, sg) in enumerate(row):
                w2 = w[e] * w[e]
                for c in range(3):
                    acc[c][t % 16] = acc[c][t % 16] + np.float64(sg) * w2 * B[e, c]
                acc[3][t % 16] = acc[3][t % 16] + w2
            rhs[v] = [_tree16(acc[c]) for c in range(3)]; diag[v] = _tree16(acc[3])
    return rhs, diag


def rhs_b(n, ii, jj, w, B):
    """mpf rhs (n, 3), diag (n) and, per row, the number of terms and sum |w^2 B| per coordinate (for the summation bound)."""
    wm, Bm = M(w), M(np.asarray(B).reshape(-1, 3))
    rhs = np.empty((n, 3), dtype=object); diag = np.empty(n, dtype=object); mag = np.empty((n, 3), dtype=object); terms = np.zeros(n, dtype=int)
    for v, row in enumerate(csr_rows(n, ii, jj)):
        terms[v] = len(row)
        diag[v] = mp.fsum(wm[e] ** 2 for e, _ in row)
        for c in range(3):
            rhs[v, c] = mp.fsum(mp.mpf(sg) * wm[e] ** 2 * Bm[e, c] for e, sg in row)
            mag[v, c] = mp.fsum(abs(wm[e] ** 2 * Bm[e, c]) for e, _ in row)
    return rhs, diag, mag, terms


def laplacian(n, ii, jj, wc):
    """Dense A' diag(wc) A over all n nodes with node 0 grounded (Build_Amatrix.m:6-13: node 1 has no column): row and column 0 are 0."""
    Lm = np.zeros((n, n))
    for e in range(len(ii)):
        i, j = ii[e], jj[e]
        Lm[i, i] += wc[e]; Lm[j, j] += wc[e]; Lm[i, j] -= wc[e]; Lm[j, i] -= wc[e]
    Lm[0, :] = 0.0; Lm[:, 0] = 0.0
    return Lm


def _tree16_rows(lanes):
    """_tree16 for an array whose axis 1 holds the 16 lanes."""
    k = np.arange(16)
    s = lanes + lanes[:, k ^ 1]
    s = s + s[:, k ^ 2]
    s = s + s[:, (k & 8) | (7 - (k & 7))]
    return s[:, 0] + s[:, 15]


def _dot3(a, b):
    """k_cg_dot: thread t of 256 sums the rows t, t + 256, ... in order, then block_reduce's tree (strides 128 ... 1)."""
    n = a.shape[0]
    sh = np.zeros((256, 3))
    for base in range(0, n, 256):
        part = a[base:base + 256] * b[base:base + 256]
        sh[:part.shape[0]] = sh[:part.shape[0]] + part
    st = 128
    while st > 0:
        sh[:st] = sh[:st] + sh[st:2 * st]
        st >>= 1
    return sh[0].copy()


@_quiet
def pcg_a(n, ii, jj, w, rhs, diag, act=(1, 1, 1), w3=False):
    """laa_pcg<W3, TRACK = W3> restated in float64 in the kernels' own order: k_cg_lap's 16 lanes per row and their butterfly, k_cg_dot's
    strided partial sums and tree, the Jacobi preconditioner, the step and breakdown rules, the probe interval (25 / 5), the stopping
    test and the cap.  Every operation is + - * /: the device result must have the same bits.  -> dict like the hook's, plus `r`
    (the recurrence residual, n x 3)."""
    w = np.asarray(w, dtype=np.float64); rhs = np.asarray(rhs, dtype=np.float64).reshape(n, 3); diag = np.asarray(diag, dtype=np.float64)
    probe, track = (5, True) if w3 else (25, False)
    W = w.reshape(-1, 3) if w3 else np.repeat((w * w)[:, None], 3, axis=1)              # operator weight per edge and coordinate
    D = diag.reshape(n, 3) if w3 else np.repeat(diag[:, None], 3, axis=1)
    rows = csr_rows(n, ii, jj)
    S = max(1, max(-(-len(r) // 16) for r in rows))
    nb = np.zeros((n, 16, S), dtype=np.int64); ed = np.zeros((n, 16, S), dtype=np.int64); ok = np.zeros((n, 16, S), dtype=bool)
    for v, row in enumerate(rows):
        if v == 0:
            continue                                                                    # the grounded node's row is not formed
        for t, (e, sg) in enumerate(row):
            nb[v, t % 16, t // 16] = jj[e] if sg < 0 else ii[e]; ed[v, t % 16, t // 16] = e; ok[v, t % 16, t // 16] = True

    def lap(p):
        acc = np.zeros((n, 16, 3))
        for s_ in range(S):
            term = W[ed[:, :, s_]] * (p[:, None, :] - p[nb[:, :, s_]])
            acc = acc + np.where(ok[:, :, s_, None], term, 0.0)
        return _tree16_rows(acc)

    def jac(r):
        z = np.where(D > 0, r / np.where(D > 0, D, 1.0), 0.0); z[0] = 0.0
        return z

    def breaks(pq, rz):
        return (not np.isfinite(pq)) or (not np.isfinite(rz)) or (pq <= 0.0 and rz > 0.0)

    x = np.zeros((n, 3)); r = rhs.copy(); r[0] = 0.0
    z = jac(r); p = z.copy()
    rz = _dot3(r, z); bnorm = _dot3(r, r)
    bad = np.zeros(3, dtype=int); rnorm = np.zeros(3)
    cg_max = min(20000, 20 * n + 200)
    done = False; k = 0
    for k in range(1, cg_max + 1):
        q = lap(p)
        pq = _dot3(p, q)
        al = np.zeros(3)
        for c in range(3):
            brk = track and (bad[c] or breaks(pq[c], rz[c]))
            al[c] = rz[c] / pq[c] if (not brk and pq[c] > 0) else 0.0
            if track and breaks(pq[c], rz[c]):
                bad[c] = 1
        x = x + al * p; r = r - al * q; z = jac(r)
        rz_new = _dot3(r, z)
        be = np.array([rz_new[c] / rz[c] if rz[c] > 0 else 0.0 for c in range(3)])
        p = z + be * p
        if track:
            bad[~np.isfinite(rz_new)] = 1
        rz = rz_new
        if k % probe == 0 or k == cg_max:
            rnorm = _dot3(r, r)
            done = not any(act[c] and not bad[c] and rnorm[c] > 1e-26 * bnorm[c] and rnorm[c] > 1e-300 for c in range(3))
            if done or k == cg_max:
                break
    badm = np.array([int(bool(act[c]) and bad[c]) for c in range(3)])
    worst = max([0.0] + [float(np.sqrt(rnorm[c] / bnorm[c])) for c in range(3) if act[c] and not badm[c] and bnorm[c] > 0])
    return dict(x=x, r=r, bad=badm, rnorm=rnorm, bnorm=bnorm, total=min(k, cg_max), unconverged=int(not done), worst=worst, cap=cg_max, probe=probe)


def pcg_b(n, ii, jj, w, rhs, w3=False):
    """The grounded systems solved by mpmath.lu_solve (n <= 40): mpf x (n, 3), row 0 = 0; a singular coordinate gives NaN."""
    w = np.asarray(w, dtype=np.float64); rhs = np.asarray(rhs, dtype=np.float64).reshape(n, 3)
    x = np.empty((n, 3), dtype=object)
    for c in range(3):
        wc = w.reshape(-1, 3)[:, c] if w3 else None
        x[0, c] = mp.mpf(0)
        if not np.all(np.isfinite(wc if w3 else w)):
            for v in range(1, n): x[v, c] = mp.nan
            continue
        A = mp.zeros(n - 1, n - 1)
        for e in range(len(ii)):
            we = mp.mpf(float(wc[e])) if w3 else mp.mpf(float(w[e])) ** 2
            i, j = int(ii[e]) - 1, int(jj[e]) - 1
            if i >= 0: A[i, i] += we
            A[j, j] += we
            if i >= 0: A[i, j] -= we; A[j, i] -= we
        b = mp.matrix([mp.mpf(float(v)) for v in rhs[1:, c]])
        try:
            sol = mp.lu_solve(A, b)
            for v in range(1, n): x[v, c] = sol[v - 1]
        except ZeroDivisionError:
            for v in range(1, n): x[v, c] = mp.nan
    return x


def true_residual_b(n, ii, jj, w, rhs, x, w3=False):
    """rhs - A' W A x (rows 1..) in mpf from a float x: (n, 3) floats, row 0 = 0."""
    w = np.asarray(w, dtype=np.float64); rhs = np.asarray(rhs, dtype=np.float64).reshape(n, 3); x = np.asarray(x, dtype=np.float64).reshape(n, 3)
    out = np.zeros((n, 3))
    for c in range(3):
        acc = [mp.mpf(float(rhs[v, c])) for v in range(n)]
        for e in range(len(ii)):
            we = mp.mpf(float(w.reshape(-1, 3)[e, c])) if w3 else mp.mpf(float(w[e])) ** 2
            i, j = ii[e], jj[e]
            d = we * ((mp.mpf(float(x[j, c])) if j > 0 else 0) - (mp.mpf(float(x[i, c])) if i > 0 else 0))
            acc[j] -= d; acc[i] += d
        acc[0] = mp.mpf(0)
        out[:, c] = [float(v) for v in acc]
    return out


def jacobi_condition(n, ii, jj, wc):
    """2-norm condition number of D^-1/2 (A' diag(wc) A) D^-1/2 over the nodes 1.. (inf when singular)."""
    Lm = laplacian(n, ii, jj, wc)[1:, 1:]
    d = np.diag(Lm)
    if not np.all(d > 0):
        return np.inf
    ev = np.linalg.eigvalsh(Lm / np.sqrt(np.outer(d, d)))
    return np.inf if ev[0] <= 0 else float(ev[-1] / ev[0])


# =================================================================================================== exp map and node update
@_quiet
def qexp_a(x):
    """laa.h qexp (Weighted_LAA.m:42-46): -> w (n, 4), theta (n); NaN -> 0."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    th = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
    f = np.sin(th / 2.0) / th
    w = np.stack([np.cos(th / 2.0), x[:, 0] * f, x[:, 1] * f, x[:, 2] * f], axis=1)
    w[np.isnan(w)] = 0.0
    return w, th


def qexp_b(x):
    """mpf w (n, 4), theta (n); a NaN row follows the NaN -> 0 rule, theta = 0 gives (1, 0, 0, 0)."""
    xf = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    w = np.empty((xf.shape[0], 4), dtype=object); th = np.empty(xf.shape[0], dtype=object)
    for v in range(xf.shape[0]):
        if not np.all(np.isfinite(xf[v])):
            w[v] = [mp.mpf(0)] * 4; th[v] = mp.nan
            continue
        t = [mp.mpf(float(u)) for u in xf[v]]
        th[v] = mp.sqrt(t[0] ** 2 + t[1] ** 2 + t[2] ** 2)
        if th[v] == 0:
            w[v] = [mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(0)]
        else:
            f = mp.sin(th[v] / 2) / th[v]
            w[v] = [mp.cos(th[v] / 2), t[0] * f, t[1] * f, t[2] * f]
    return w, th


def qmul_rows_b(Q, w):
    Qm = M(np.asarray(Q).reshape(-1, 4))
    out = np.empty(Qm.shape, dtype=object)
    for v in range(Qm.shape[0]):
        out[v] = [mp.nan] * 4 if any(mp.isnan(t) or mp.isinf(t) for t in Qm[v]) else qmul_b(list(Qm[v]), list(w[v]))
    return out


# =================================================================================================== weights
@_quiet
def weights_a(RS, thresh, wmax=1e4, wmin=1e-4):
    """k_weights (DESC.m:298-303): 1 / RS^0.75 clipped at wmax; wmin where RS > thresh (strict)."""
    RS = np.asarray(RS, dtype=np.float64)
    w = 1.0 / np.power(RS, 0.75)
    w = np.where(w > wmax, wmax, w)
    return np.where(RS > thresh, wmin, w)


def weights_b(RS, thresh, wmax=1e4, wmin=1e-4):
    RS = np.asarray(RS, dtype=np.float64)
    out = np.empty(RS.shape, dtype=object)
    for k, v in np.ndenumerate(RS):
        if v == -np.inf and not v > thresh:
            out[k] = mp.mpf(0)                                    # pow(-inf, 0.75) = +inf (C99): 1 / inf
        elif np.isnan(v) or v < 0:
            out[k] = mp.nan
        elif v > thresh:
            out[k] = mp.mpf(wmin)
        elif v == 0:
            out[k] = mp.mpf(wmax)
        else:
            t = 1 / mp.power(mp.mpf(float(v)), mp.mpf(0.75)) if np.isfinite(v) else mp.mpf(0)
            out[k] = mp.mpf(wmax) if t > wmax else t
    return out


@_quiet
def edge_residual_sq_a(ii, jj, x, B):
    """laa.h edge_residual_sq: node 0 grounded."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3); B = np.asarray(B, dtype=np.float64).reshape(-1, 3)
    s = np.zeros(len(ii))
    for c in range(3):
        ax = np.where(jj > 0, x[jj, c], 0.0) - np.where(ii > 0, x[ii, c], 0.0)
        d = ax - B[:, c]
        s = s + d * d
    return s


@_quiet
def irls_weights_a(ii, jj, x, B, mode, sigma):
    """k_irls_weights (RobustMeanSO3Graph.m:169-170, L12.m:169-171)."""
    s = edge_residual_sq_a(ii, jj, x, B)
    if mode == GM:
        return sigma / (s + sigma * sigma)
    w = 1.0 / np.power(np.sqrt(s), 0.75)
    return np.where(w > 1e4, 1e4, w)


def irls_weights_b(ii, jj, x, B, mode, sigma):
    xm, Bm = M(np.asarray(x).reshape(-1, 3)), M(np.asarray(B).reshape(-1, 3))
    out = np.empty(len(ii), dtype=object); sg = mp.mpf(float(sigma))
    for e in range(len(ii)):
        s = mp.mpf(0)
        for c in range(3):
            ax = (xm[jj[e], c] if jj[e] > 0 else 0) - (xm[ii[e], c] if ii[e] > 0 else 0)
            s += (ax - Bm[e, c]) ** 2
        if mode == GM:
            out[e] = sg / (s + sg * sg)
        elif s == 0:
            out[e] = mp.mpf(1e4)
        else:
            t = 1 / mp.power(mp.sqrt(s), mp.mpf(0.75))
            out[e] = mp.mpf(1e4) if t > 1e4 else t
    return out


# =================================================================================================== quantile
@_quiet
def quantile_a(x, p):
    """MATLAB quantile(x, p) as device_quantile evaluates it: Hazen position p m + 0.5, a + fr (b - a) on the sorted vector."""
    xs = np.sort(np.asarray(x, dtype=np.float64)); m = xs.size
    pos = p * float(m) + 0.5
    if pos <= 1.0:
        return xs[0]
    if pos >= float(m):
        return xs[-1]
    k0 = int(np.floor(pos)) - 1; fr = pos - np.floor(pos)
    a, b = xs[k0], xs[k0 + 1]
    return a + fr * (b - a)


def quantile_b(x, p):
    """The same Hazen interpolation at 50 digits on the same doubles: mpf value, and the two order statistics it lies between."""
    xs = np.sort(np.asarray(x, dtype=np.float64)); m = xs.size
    pos = mp.mpf(float(p)) * m + mp.mpf(0.5)
    if pos <= 1:
        return mp.mpf(float(xs[0])), xs[0], xs[0]
    if pos >= m:
        return mp.mpf(float(xs[-1])), xs[-1], xs[-1]
    k0 = int(mp.floor(pos)) - 1; fr = pos - mp.floor(pos)
    a, b = mp.mpf(float(xs[k0])), mp.mpf(float(xs[k0 + 1]))
    return a + fr * (b - a), xs[k0], xs[k0 + 1]


@_quiet
def quantile_plan(x, p):
    """Which path device_quantile takes: 'min' / 'max' / 'const' (early returns) or 'bins' with the two bins of the order statistics
    and `need`, the number of values they hold (need > cap -> the exact host path)."""
    x = np.asarray(x, dtype=np.float64); m = x.size
    pos = p * float(m) + 0.5
    if pos <= 1.0: return dict(path="min")
    if pos >= float(m): return dict(path="max")
    lo, hi = x.min(), x.max()
    if not hi > lo: return dict(path="const")
    k0 = int(np.floor(pos)) - 1
    scale = float(QBINS) / (hi - lo) * (1.0 - 1e-12)
    t = (x - lo) * scale
    b = np.where(np.isnan(t), 0.0, np.clip(np.where(np.isnan(t), 0.0, t), -1.0, float(QBINS))).astype(np.int64)
    b = np.clip(b, 0, QBINS - 1)
    bs = np.sort(b)
    b0, b1 = int(bs[k0]), int(bs[k0 + 1])
    need = int((b == b0).sum() + ((b == b1).sum() if b1 != b0 else 0))
    return dict(path="bins", b0=b0, b1=b1, need=need, k0=k0, last_of_bin=bool(k0 + 1 == (b <= b0).sum()))


# =================================================================================================== projection
@_quiet
def project_det_a(rij):
    """k_irls_project's determinant of RR = Rij' in its bracketing."""
    R = np.asarray(rij, dtype=np.float64).reshape(-1, 9)
    a = [R[:, (k % 3) * 3 + k // 3] for k in range(9)]          # a[r + 3c] = rij[c + 3r]
    return a[0] * (a[4] * a[8] - a[7] * a[5]) - a[3] * (a[1] * a[8] - a[7] * a[2]) + a[6] * (a[1] * a[5] - a[4] * a[2])


def project_status(rij, margin=1e-12):
    """IRLS_GM.m:82-93 from NumPy's SVD: status 3 det <= 0, 2 all |s - 1| >= 0.1, 1 all >= 0.01, else 0; s (m, 3) descending;
    decided[e]: no singular value within `margin` of a threshold."""
    R = np.asarray(rij, dtype=np.float64).reshape(-1, 9)
    det = project_det_a(R)
    s = np.array([np.linalg.svd(R[e].reshape(3, 3), compute_uv=False) for e in range(R.shape[0])]).reshape(-1, 3)
    d = np.abs(s - 1.0)
    status = np.where(det <= 0, 3, np.where(np.all(d >= 0.1, axis=1), 2, np.where(np.all(d >= 0.01, axis=1), 1, 0)))
    decided = (np.abs(d - 0.1).min(axis=1) > margin) & (np.abs(d - 0.01).min(axis=1) > margin)      # det is restated exactly: always decided
    return status, det, s, decided


def project_b(rij):
    """U round(S) V' of RR = Rij' from mpmath.svd, round half away from zero: mpf (m, 9) column-major."""
    R = np.asarray(rij, dtype=np.float64).reshape(-1, 9)
    out = np.empty((R.shape[0], 9), dtype=object)
    for e in range(R.shape[0]):
        A = mp.matrix(3, 3)
        for r in range(3):
            for c in range(3):
                A[r, c] = mp.mpf(float(R[e, c + 3 * r]))          # RR(r, c) = Rij(c, r); Rij column-major: (c, r) at c + 3r
        U, S, V = mp.svd_r(A)
        sv = []
        for k in range(3):                                       # a singular value that is a double to 30 digits IS that double (0.5, 1.5)
            f = mp.mpf(float(S[k]))
            sv.append(f if abs(S[k] - f) < mp.mpf(10) ** -30 else S[k])
        rs = mp.diag([mp.floor(v + mp.mpf(0.5)) for v in sv])
        P = U * rs * V
        for r in range(3):
            for c in range(3):
                out[e, r + 3 * c] = P[r, c]
    return out


# =================================================================================================== the few-ulp rule
def few_ulp(dev, a, b, mag=None):
    """Per component: device error against (b) <= 4 x the error of (a) against (b) + 4 ulp of the component's magnitude (mag: float
    array broadcastable to the shape; default |b|).  Compared where (a) is finite.  -> dict(ok, worst_ratio = max error / allowance,
    worst_ulp = max device error in ulp of the magnitude, worst_a_ulp = the same for (a))."""
    dev, a = np.asarray(dev, dtype=np.float64), np.asarray(a, dtype=np.float64)
    e_dev, e_a = mp_abs_err(dev, b), mp_abs_err(a, b)
    fin = np.isfinite(a) & np.isfinite(dev) & ~np.isnan(e_a)          # non-finite positions are compared below, exactly
    magf = np.abs(to_float(b)) if mag is None else np.broadcast_to(np.asarray(mag, dtype=np.float64), a.shape)
    with np.errstate(all="ignore"):
        ulp = np.spacing(np.where(np.isfinite(magf), np.abs(magf), 0.0))
        allow = 4.0 * e_a + 4.0 * ulp
        ok = np.where(fin, e_dev <= allow, True)
        ratio = np.where(fin, e_dev / allow, 0.0); u_dev = np.where(fin, e_dev / ulp, 0.0); u_a = np.where(fin, e_a / ulp, 0.0)
    nonfinite_same = bool(np.array_equal(np.isnan(dev), np.isnan(a)) and np.array_equal(np.isinf(dev), np.isinf(a)) and
                          np.array_equal(np.sign(dev[np.isinf(a)]), np.sign(a[np.isinf(a)])))
    return dict(ok=bool(np.all(ok)) and nonfinite_same, nonfinite_same=nonfinite_same, worst_ratio=float(np.nanmax(ratio, initial=0.0)),
                worst_ulp=float(np.nanmax(u_dev, initial=0.0)), worst_a_ulp=float(np.nanmax(u_a, initial=0.0)),
                where=np.argwhere(~ok))

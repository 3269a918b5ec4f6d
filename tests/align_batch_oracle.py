"""NumPy / plain-Python restatement of what include/desc_amd.h fixes for desc_align_batch_run: the workgroup's summation order (the
Gram sums of pass 1 and mean_error), the median rule, the one-sided Jacobi SVD and the projection behind R_align.  Every sum is written
out in ascending order from 0.0; nothing here calls BLAS or LAPACK."""
import math

import numpy as np

_LANE = np.arange(256)


def wg_sum(partials):
    """The workgroup's fixed reduction of 256 per-thread partials (leading axis): inside a wave the butterfly of group_sum<64> -- every
    lane adds the value of lane ^ 1, ^ 2, ^ 7 (the half-row mirror), ^ 15 (the row mirror), ^ 16, ^ 32 in turn; IEEE addition commutes,
    so which operand comes first changes no bit --, then ((wave 0 + wave 1) + wave 2) + wave 3."""
    v = np.array(partials, dtype=np.float64)
    assert v.shape[0] == 256
    for x in (1, 2, 7, 15, 16, 32):
        v = v + v[_LANE ^ x]
    return ((v[0] + v[64]) + v[128]) + v[192]


def strided_partials(values):
    """Thread t's running sum of values[t], values[t + 256], ... from 0.0 (leading axis: the nodes)."""
    values = np.asarray(values, dtype=np.float64)
    part = np.zeros((256,) + values.shape[1:])
    for base in range(0, values.shape[0], 256):
        chunk = values[base:base + 256]
        part[:chunk.shape[0]] = part[:chunk.shape[0]] + chunk
    return part


def mean_error(err):
    err = np.asarray(err, dtype=np.float64)
    return float(wg_sum(strided_partials(err)) / float(err.shape[0]))


def median_error(err):
    """MATLAB's median of non-negative values: the order statistic of rank (n + 1) / 2, or a + (b - a) / 2 of the two middle ones."""
    s = np.sort(np.asarray(err, dtype=np.float64))
    n = s.shape[0]
    if n % 2:
        return float(s[(n - 1) // 2])
    a, b = s[n // 2 - 1], s[n // 2]
    return float(a + (b - a) / 2.0)


def gram(R_est, R_gt):
    """A = sum_k R_est_k' R_gt_k in the device's order: entry (r, c) of a node is sum_a R_est(a, r) R_gt(a, c) in ascending a from 0.0."""
    E, G = np.asarray(R_est, dtype=np.float64), np.asarray(R_gt, dtype=np.float64)
    n = E.shape[2]
    node = np.zeros((n, 3, 3))
    for r in range(3):
        for c in range(3):
            s = np.zeros(n)
            for a in range(3):
                s = s + E[a, r, :] * G[a, c, :]
            node[:, r, c] = s
    return wg_sum(strided_partials(node))


def svd3(A):
    """The one-sided Jacobi SVD of a 3x3 matrix (irls_math.h): A V = U S.  Returns the columns of U S, the columns of V, and s, sorted
    descending."""
    a = [[float(A[r][k]) for r in range(3)] for k in range(3)]            # a[k]: column k
    v = [[1.0 if r == k else 0.0 for r in range(3)] for k in range(3)]
    for _ in range(40):
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            al = be = ga = 0.0
            for r in range(3):
                al += a[p][r] * a[p][r]
                be += a[q][r] * a[q][r]
                ga += a[p][r] * a[q][r]
            if not (abs(ga) > 1e-300 and abs(ga) > 1e-17 * math.sqrt(al * be)):
                continue
            rotated = True
            zeta = (be - al) / (2.0 * ga)
            t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
            c = 1.0 / math.sqrt(1.0 + t * t)
            sn = c * t
            for r in range(3):
                ap, aq = a[p][r], a[q][r]
                a[p][r], a[q][r] = c * ap - sn * aq, sn * ap + c * aq
                vp, vq = v[p][r], v[q][r]
                v[p][r], v[q][r] = c * vp - sn * vq, sn * vp + c * vq
        if not rotated:
            break
    s = [math.sqrt(a[k][0] * a[k][0] + a[k][1] * a[k][1] + a[k][2] * a[k][2]) for k in range(3)]
    for i in range(2):
        for k in range(2 - i):
            if s[k] < s[k + 1]:
                s[k], s[k + 1] = s[k + 1], s[k]
                a[k], a[k + 1] = a[k + 1], a[k]
                v[k], v[k + 1] = v[k + 1], v[k]
    return a, v, s


def project(A):
    """U diag(1, 1, det(U V')) V' of the 3x3 matrix A, the third left vector as det(V) (u1 x u2)."""
    a, v, _ = svd3(A)
    n1 = 0.0
    for r in range(3):
        n1 += a[0][r] * a[0][r]
    n1 = math.sqrt(n1)
    u1 = [a[0][r] / n1 for r in range(3)]
    d12 = 0.0
    for r in range(3):
        d12 += u1[r] * a[1][r]
    u2, n2 = [0.0] * 3, 0.0
    for r in range(3):
        u2[r] = a[1][r] - d12 * u1[r]
        n2 += u2[r] * u2[r]
    n2 = math.sqrt(n2)
    u2 = [u2[r] / n2 for r in range(3)]
    (v0, v1, v2), (v3, v4, v5), (v6, v7, v8) = v                          # v[k] of the device: column-major
    dv = v0 * (v4 * v8 - v7 * v5) - v3 * (v1 * v8 - v7 * v2) + v6 * (v1 * v5 - v4 * v2)
    sg = -1.0 if dv < 0 else 1.0
    u3 = [sg * (u1[1] * u2[2] - u1[2] * u2[1]), sg * (u1[2] * u2[0] - u1[0] * u2[2]), sg * (u1[0] * u2[1] - u1[1] * u2[0])]
    R = np.zeros((3, 3))
    for c in range(3):
        for r in range(3):
            R[r, c] = (u1[r] * v[0][c] + u2[r] * v[1][c]) + u3[r] * v[2][c]
    return R


def project_blocks(A9):
    """project() of count column-major blocks (count x 9) -> count x 9, column-major."""
    A9 = np.asarray(A9, dtype=np.float64).reshape(-1, 9)
    return np.array([project(blk.reshape(3, 3, order="F")).reshape(-1, order="F") for blk in A9]).reshape(-1, 9)


def abs_acos_ext(x):
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    inside = np.abs(x) <= 1
    out[inside] = np.arccos(x[inside])
    out[x > 1] = np.arccosh(x[x > 1])
    out[x < -1] = np.hypot(np.pi, np.arccosh(-x[x < -1]))
    return out


def rotation_alignment(R_est, R_gt):
    """The whole call restated: (R_out, R_align, mean_error, median_error, err)."""
    E, G = np.asarray(R_est, dtype=np.float64), np.asarray(R_gt, dtype=np.float64)
    Ra = project(gram(E, G))
    n = E.shape[2]
    R_out = np.zeros((3, 3, n), order="F")
    for r in range(3):
        for c in range(3):
            s = np.zeros(n)
            for j in range(3):
                s = s + E[r, j, :] * Ra[j, c]
            R_out[r, c, :] = s
    tr = np.zeros(n)
    for c in range(3):                                                    # column-major order
        for r in range(3):
            tr = tr + G[r, c, :] * R_out[r, c, :]
    err = abs_acos_ext((tr - 1.0) / 2.0) / np.pi * 180
    return R_out, Ra, mean_error(err), median_error(err), err

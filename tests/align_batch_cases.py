"""The seeded problems of tests/test_gpu_align_batch.py and tests/test_align_batch_host.py: pairs (R_est, R_gt) of Fortran-ordered 3x3xn
arrays, with Rotation_Alignment's answer for each computed once and shared (treat everything here as read-only).

Sizes: n = 1, 2, 3 (the median of one, of two, odd); 255, 256, 257, 513 (the 256-thread stride edge, and three strides with remainder 1);
the batch MIXED of sizes [1, 257, 2, 100, 64] (sizes differ inside one launch); MANY, 300 problems of n = 5 (more workgroups than the
256 compute units).
Kinds: noisy (R_gt_k * a rotation by 3 degrees about a random axis * g, one Haar g per problem), exact (R_gt_k * g), garbage
(independent Haar estimates; also at n = 7: det A < 0 occurs among the garbage problems of n = 3 and n = 7), mixed (noisy, every fourth
node garbage), constant (every node the same pair of rotations, so all errors are the same bits), two-class (half the nodes one pair, the
rest another, at n = 256 (128 / 128) and n = 257 (129 / 128): the median straddles, or sits inside, a run of duplicates)."""
import functools

import numpy as np

GAP_MIN = 1e-2           # R_align is ill-defined as (s2 + sign(det A) s3) / s1 -> 0; every case here stays above
# What tests/align_batch_oracle.py (Jacobi SVD, the device's summation orders) differs from Rotation_Alignment (LAPACK, NumPy's sums) by on
# the cases below, measured on the CPU and rounded up: max abs differences; err over the nodes whose reference error exceeds 1e-3
# degrees; mean and median over the problems whose reference median exceeds 1e-3 degrees.  The GPU test allows 16 times as much: the
# margin for the device's acos and sqrt against libm's, a few ulps.
MEASURED = dict(R_align=1.9e-14, R_out=1.9e-14, err=8.0e-12, mean=3.5e-12, median=3.5e-12)
TOL = {k: 16 * v for k, v in MEASURED.items()}
# R_est_k = R_gt_k * g: every error is at most 64 ulps of 1 in the trace, sqrt(2 * 64 * 2^-53) rad = 6.8e-6 degrees.  The problems whose
# reference median lies below 1e-3 degrees are of this sort (exact, constant): their mean and median are compared through this bound.
EXACT_MAX = (2 * 64 * 2.0 ** -53) ** 0.5 * 180 / np.pi
SIZES = (1, 2, 3, 255, 256, 257, 513)
KINDS = ("noisy", "exact", "garbage", "mixed", "constant")


def haar(rng, count):
    """count Haar rotations (count, 3, 3): QR of a normal block with R's diagonal made positive, the determinant's sign on a column."""
    Q, R = np.linalg.qr(rng.standard_normal((count, 3, 3)))
    Q = Q * np.sign(np.diagonal(R, axis1=1, axis2=2))[:, None, :]
    Q[:, :, 2] *= np.linalg.det(Q)[:, None]
    return Q


def small(rng, count, degrees=3.0):
    """count rotations by `degrees` about random axes (Rodrigues)."""
    ax = rng.standard_normal((count, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    K = np.zeros((count, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def _f(stack):
    """(n, 3, 3) -> Fortran-ordered 3x3xn."""
    return np.asfortranarray(np.transpose(stack, (1, 2, 0)))


def problem(kind, n, seed):
    rng = np.random.default_rng(seed)
    G, g = haar(rng, n), haar(rng, 1)[0]
    if kind == "exact":
        E = G @ g
    elif kind == "noisy":
        E = G @ small(rng, n) @ g
    elif kind == "garbage":
        E = haar(rng, n)
    elif kind == "mixed":
        E = G @ small(rng, n) @ g
        E[::4] = haar(rng, E[::4].shape[0])
    elif kind == "constant":
        E, G = np.repeat(haar(rng, 1), n, axis=0), np.repeat(G[:1], n, axis=0)
    elif kind == "two-class":
        h = (n + 1) // 2
        e, c = haar(rng, 2), haar(rng, 2)
        E = np.concatenate([np.repeat(e[:1], h, axis=0), np.repeat(e[1:], n - h, axis=0)])
        G = np.concatenate([np.repeat(c[:1], h, axis=0), np.repeat(c[1:], n - h, axis=0)])
    else:
        raise ValueError(kind)
    return _f(E), _f(G)


def _build():
    out = {}
    for i, kind in enumerate(KINDS):
        for n in SIZES:
            out[f"{kind}-{n}"] = problem(kind, n, 1000 * (i + 1) + n)
    for t, (s3, s7) in enumerate(((7000, 7100), (7015, 7102), (7037, 7121))):      # seeds 7015, 7037, 7102, 7121: det A < 0 (the host test asserts it)
        out[f"garbage-3-{t}"] = problem("garbage", 3, s3)
        out[f"garbage-7-{t}"] = problem("garbage", 7, s7)
    # the pairs' seeds were chosen so that the two classes' relative rotations lie about 150 degrees apart: A = n1 Q1 + n2 Q2 then has
    # the gap 2 cos(75 degrees) = 0.5, far above GAP_MIN, and the errors are far from acos's ill-conditioned end
    out["two-class-256"] = problem("two-class", 256, 8656)
    out["two-class-257"] = problem("two-class", 257, 8657)
    return out


SINGLE = _build()                                                # name -> (R_est, R_gt); one batch in the order of the dict
MIXED = [problem(kind, n, 9000 + n) for kind, n in (("garbage", 1), ("noisy", 257), ("exact", 2), ("mixed", 100), ("noisy", 64))]
MANY = [problem(KINDS[b % 4], 5, 20000 + b) for b in range(300)]


def gram(E, G):
    """A = sum_k R_est_k' R_gt_k and its gap (s2 + sign(det A) s3) / s1."""
    A = np.einsum("abk,ack->bc", E, G)
    s = np.linalg.svd(A, compute_uv=False)
    return A, (s[1] + np.sign(np.linalg.det(A)) * s[2]) / s[0]


def every_problem():
    """(label, R_est, R_gt) of every problem of SINGLE, MIXED and MANY."""
    for name, (E, G) in SINGLE.items():
        yield name, E, G
    for b, (E, G) in enumerate(MIXED):
        yield f"mixed[{b}]", E, G
    for b, (E, G) in enumerate(MANY):
        yield f"many[{b}]", E, G


@functools.lru_cache(maxsize=None)
def reference(which):
    """Rotation_Alignment's (R_out, R_align, mean, median, err) per problem of 'single' | 'mixed' | 'many', computed once."""
    from desc_amd import Rotation_Alignment
    probs = dict(single=list(SINGLE.values()), mixed=MIXED, many=MANY)[which]
    out = []
    for E, G in probs:
        R_out, R_align, mean, median = Rotation_Alignment(E, G)
        x = (np.einsum("abk,abk->k", G, R_out) - 1.0) / 2.0
        err = np.where(np.abs(x) <= 1, np.arccos(np.clip(x, -1, 1)), np.abs(np.arccos(x.astype(complex)))) / np.pi * 180   # its own line
        out.append((R_out, R_align, mean, median, err))
    return tuple(out)

"""IRLS_GM / IRLS_L12 without a GPU: known answers of the NumPy restatement (tests/irls_oracle.py) and the C ABI's structs."""
import ctypes as C

import numpy as np
import pytest
import scipy.optimize

from desc_amd import Rotation_Alignment, _lib
from desc_amd.models import Uniform_Topology
from oracle.refine_oracle import R2Q
from tests.irls_oracle import amatrix, irls_oracle, l1decode_pd, largest_component, project, tree_start


def random_rotations(k, rng):
    Q = np.linalg.qr(rng.standard_normal((k, 3, 3)))[0]
    Q[np.linalg.det(Q) < 0, :, 0] *= -1
    return np.ascontiguousarray(np.transpose(Q, (1, 2, 0)))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_l1decode_pd_reaches_the_lp_optimum(seed):
    """With 50 primal-dual steps l1decode_pd solves min |y - A x|_1; linprog on the LP form gives the optimum."""
    rng = np.random.default_rng(seed)
    mo = Uniform_Topology(12, 0.6, 0.2, 0.1, "uniform", seed=seed)
    I = mo.Ind.T
    N = int(I.max())
    A = amatrix(I, N)
    y = rng.standard_normal(I.shape[1]) * 0.3
    x = l1decode_pd(np.zeros(N - 1), A, y, 1e-10, 50)
    m, n = A.shape
    Ad = A.toarray()
    c = np.concatenate([np.zeros(n), np.ones(m)])
    A_ub = np.block([[Ad, -np.eye(m)], [-Ad, -np.eye(m)]])
    b_ub = np.concatenate([y, -y])
    lp = scipy.optimize.linprog(c, A_ub=A_ub, b_ub=b_ub, bounds=[(None, None)] * n + [(0, None)] * m, method="highs")
    opt = lp.fun
    got = np.abs(y - Ad @ x).sum()
    assert abs(got - opt) <= 1e-6 * opt, (got, opt)


def _quat(rng, k):
    q = rng.standard_normal((k, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True); q[:, 0] = np.abs(q[:, 0])
    return q


def test_tree_start_needs_a_second_pass_and_follows_the_row_order():
    """Rows (4,5), (3,4), (2,3), (1,2): one pass reaches node 2 only at the last row, so passes 2-4 add one node each.  Listing the
    same edges from node 1 outward reaches all of them in one pass; a row order in which an edge seeds a later one in the same pass
    also does."""
    rng = np.random.default_rng(3)
    I = np.array([[4, 3, 2, 1], [5, 4, 3, 2]])
    QQ = _quat(rng, 4)
    Q, passes, seq = tree_start(I, QQ, 5)
    assert passes == 4 and seq == [3, 2, 1, 0]
    Q2, passes2, seq2 = tree_start(I[:, ::-1], QQ[::-1], 5)
    assert passes2 == 1 and seq2 == [0, 1, 2, 3]
    assert np.abs(Q - Q2).max() < 1e-15                                     # same tree, same products
    # a graph with two trees: which one is taken depends on the row order
    I3 = np.array([[1, 1, 2, 3], [2, 3, 3, 4]])
    QQ3 = _quat(rng, 4)
    _, _, s_a = tree_start(I3, QQ3, 4)
    _, _, s_b = tree_start(I3[:, [2, 0, 1, 3]], QQ3[[2, 0, 1, 3]], 4)
    assert s_a == [0, 1, 3]                                                   # (1,2), (1,3), (3,4)
    assert s_b == [1, 2, 3]                                                   # (1,2), (1,3) -- listed as rows 2, 3 -- then (3,4); (2,3) skipped


def test_projection_check_needs_all_three_singular_values():
    R = random_rotations(3, np.random.default_rng(0))
    RR = R.copy()
    RR[:, :, 0] = R[:, :, 0] @ np.diag([1.5, 1.0, 1.0])                       # one value off: projected silently
    RR[:, :, 1] = R[:, :, 1] * 1.05                                           # all three off by 0.05: warning
    P, warned = project(RR)
    assert warned == 1
    for e in range(3):
        assert np.abs(P[:, :, e] - R[:, :, e]).max() < 1e-12
    RR[:, :, 2] = R[:, :, 2] * 1.2                                            # all three off by 0.2: error naming edge 3
    with pytest.raises(ValueError, match=r"svd\(RR\(:,:,3\)\)"):
        project(RR)
    RR[:, :, 1] = -R[:, :, 1]
    with pytest.raises(ValueError, match=r"det\(RR\(:,:,2\)\)"):
        project(RR)


def test_component_tie_rule_and_nan_placement():
    """Two components of 3 nodes and an untouched id: the one holding node 2 comes first (node 1 is isolated)."""
    Ind = np.array([[2, 3], [3, 4], [2, 4], [5, 6], [6, 8], [5, 8]])
    nodes, mask = largest_component(Ind, 8)
    assert list(nodes) == [1, 2, 3] and list(mask) == [True] * 3 + [False] * 3
    rng = np.random.default_rng(1)
    Rabs = random_rotations(8, rng)
    Rij = np.stack([Rabs[:, :, j - 1] @ Rabs[:, :, i - 1].T for i, j in Ind], axis=2)
    R, R1, tr = irls_oracle(Rij, Ind, "GM")
    assert np.isnan(R[:, :, [0, 4, 5, 6, 7]]).all() and not np.isnan(R[:, :, [1, 2, 3]]).any()
    assert tr["comp_nodes"] == 3 and tr["comp_edges"] == 3


def test_self_consistent_gap_comes_from_one_edge_near_pi():
    """Pins the reason for the looser R_l1 bound of the self-consistent graph in tests/test_gpu_irls.py: one edge turns by nearly pi
    (cos(angle/2) = 4.9e-5 after projection), and R2Q's division by cos(angle/2) makes the oracle's own R_l1 move by more than 1e-8
    when that block changes by one unit in the last place, while the same change to the 20 edges farthest from pi does nothing."""
    mo = Uniform_Topology(100, 0.3, 0.2, 0.1, "self-consistent", seed=2)
    P, _ = project(np.transpose(mo.RijMat, (1, 0, 2)))
    q0 = R2Q(P)[:, 0]
    e = int(np.argmin(q0))
    assert q0[e] < 1e-4 and np.sort(q0)[1] > 1e-3
    _, R1, _ = irls_oracle(mo.RijMat, mo.Ind, "GM")
    eps = np.finfo(np.float64).eps

    def moved(edges):
        d = 0.0
        for f in (1 + eps, 1 - eps / 2):
            Rij = mo.RijMat.copy()
            Rij[:, :, edges] *= f
            d = max(d, float(np.abs(irls_oracle(Rij, mo.Ind, "GM")[1] - R1).max()))
        return d

    assert moved([e]) > 1e-8
    assert moved(np.argsort(-q0)[:20]) < 1e-12


@pytest.mark.parametrize("mode", ["GM", "L12"])
def test_noiseless_graph_is_recovered(mode):
    mo = Uniform_Topology(40, 0.4, 0.0, 0.0, "uniform", seed=4)
    R, R1, tr = irls_oracle(mo.RijMat, mo.Ind, mode)
    R_out, _, _, _ = Rotation_Alignment(R, mo.R_orig)
    assert np.abs(R_out - mo.R_orig).max() < 1e-10                          # entrywise, after the global alignment
    i, j = mo.Ind[:, 0] - 1, mo.Ind[:, 1] - 1
    rel = np.einsum("abk,cbk->ack", R[:, :, i], R[:, :, j])                 # the model's R_ij = R_i R_j'
    assert np.abs(rel - mo.RijMat).max() < 1e-10
    assert tr["ill"] == 0 and tr["stuck"] == 0


def test_ctypes_struct_sizes():
    assert C.sizeof(_lib.IrlsParams) == 4 * 4 + 8 + 8 + 8
    assert C.sizeof(_lib.IrlsInfo) == 2 * 8 + 2 * 4 + 2 * 8 + 8 * 4 + 8 + 7 * 8
    for k in ("R_init", "order", "sigma_deg"):
        assert hasattr(_lib.IrlsParams, k)


def test_quaternion_input_is_refused():
    from desc_amd import IRLS_GM
    with pytest.raises(ValueError, match="quaternion"):
        IRLS_GM(np.zeros((4, 3)), np.array([[1, 2], [2, 3], [1, 3]]))

"""GPU parity of IRLS_GM / IRLS_L12 (Algorithms/IRLS_GM.m, IRLS_L12.m) against the NumPy / SciPy restatement (tests/irls_oracle.py).
Tolerances: R_l1 1e-9 (the primal-dual Newton systems by PCG to |r| <= 1e-13 |b| against a dense LU), R 1e-7 (PCG normal
equations against a dense Cholesky, as the refinement and MPLS tests).

Two graphs have an edge whose relative rotation is close to pi, and there the reference's own arithmetic amplifies round-off:
R2Q (BoxMedianSO3Graph.m:55-59) takes QQ(:,1) = sqrt((trace + 1)/2), which is cos(angle/2), and divides the vector part by it.
A difference of one unit in the last place in that edge's projected block -- what the device's Jacobi SVD and LAPACK's SVD leave
between them -- then moves the L1 estimate far more than the difference between the device's CG and the oracle's LU does.
* self-consistent: edge 103 (Ind = [4 7]) turns by pi - 9.9e-5, cos(angle/2) = 4.9e-5 after projection.  Scaling that one block
  by (1 + eps) or (1 - eps/2) moves the oracle's own R_l1 by 4.1e-8 and 8.2e-8; the same scaling of the 20 edges farthest from pi
  moves it by 9e-16 (pinned by tests/test_irls_host.py).  Measured GPU gap in R_l1: 8.2e-8.  Bound: 2e-7.
* adv: edge 113 (Ind = [3 100]) turns by pi - 4.0e-4, cos(angle/2) = 2.0e-4.  Random 2e-16 relative perturbations of that block
  moved the oracle's own R_l1 by up to 1.2e-9.  Measured GPU gap in R_l1: 9.3e-12.  Bound: 1e-8, set above that sensitivity
  rather than at it, so that a change of rounding in the projection cannot break the test while the solvers still agree.
q04 has such an edge too (cos(angle/2) = 1.7e-4), but the oracle's R_l1 moves by only 1.6e-11 under random 2e-16 perturbations of
all its blocks, and 1e-9 holds.  Iteration counts, primal-dual step counts, early
returns and the warned-edge count agree exactly on every graph."""
import os
import sys

import numpy as np
import pytest

from desc_amd import IRLS_GM, IRLS_L12, Rotation_Alignment, _lib
from desc_amd.models import Nonuniform_Topology, Uniform_Topology
from tests.irls_oracle import irls_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = {"GM": IRLS_GM, "L12": IRLS_L12}


def random_rotations(k, rng):
    Q = np.linalg.qr(rng.standard_normal((k, 3, 3)))[0]
    Q[np.linalg.det(Q) < 0, :, 0] *= -1
    return np.ascontiguousarray(np.transpose(Q, (1, 2, 0)))


def nan_equal_max(a, b):
    assert np.array_equal(np.isnan(a), np.isnan(b))
    k = ~np.isnan(a)
    return float(np.abs(a[k] - b[k]).max()) if k.any() else 0.0


def check(RijMat, Ind, mode, tol_l1=1e-9, tol=1e-7, **kw):
    R, info = FN[mode](RijMat, Ind, return_info=True, **kw)
    okw = {k: v for k, v in kw.items() if k in ("Rinit", "SIGMA", "MaxIterations")}
    ref, ref1, tr = irls_oracle(RijMat, Ind, mode, **okw)
    assert info["l1_iters"] == tr["l1_iters"] and info["irls_iters"] == tr["irls_iters"], (info, tr["l1_iters"], tr["irls_iters"])
    assert (info["pd_steps"], info["pd_ill"], info["pd_stuck"]) == (tr["steps"], tr["ill"], tr["stuck"])
    assert info["cg_unconverged"] == 0
    assert info["comp_nodes"] == tr["comp_nodes"] and info["comp_edges"] == tr["comp_edges"]
    assert info["warned_edges"] == tr["warned"]
    d1 = nan_equal_max(info["R_l1"], ref1)
    d = nan_equal_max(R, ref)
    assert d1 <= tol_l1, d1
    assert d <= tol, d
    return R, info, tr


GRAPHS = [     # name, model, R_l1 bound; smallest cos(angle/2) of a projected edge in the comment
    ("uniform", lambda: Uniform_Topology(30, 0.5, 0.1, 0.05, "uniform", seed=1), 1e-9),                     # 1.6e-2
    ("self-consistent", lambda: Uniform_Topology(100, 0.3, 0.2, 0.1, "self-consistent", seed=2), 2e-7),     # 4.9e-5: see the docstring
    ("adv", lambda: Nonuniform_Topology(150, 0.3, 0.3, 0.5, 0.1, 0.2, "adv", seed=3), 1e-8),                # 2.0e-4: see the docstring
    ("q04", lambda: Uniform_Topology(300, 0.2, 0.4, 0.1, "uniform", seed=4), 1e-9),                         # 1.7e-4, sensitivity 1.6e-11
]


@pytest.mark.parametrize("mode", ["GM", "L12"])
@pytest.mark.parametrize("name,make,tol_l1", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_parity_with_oracle(name, make, tol_l1, mode):
    mo = make()
    _, info, tr = check(mo.RijMat, mo.Ind, mode, tol_l1=tol_l1)
    assert info["pd_ill"] == 0 and info["pd_stuck"] == 0


@pytest.mark.parametrize("mode", ["GM", "L12"])
def test_projection_of_blocks_that_are_not_rotations(mode):
    """Three blocks scaled by 1.03 (all singular values off by 0.03: the warning path, projected back to the rotation) and one block
    with a single singular value of 1.6 (no warning; round(S) makes it 2, so U round(S) V' is not a rotation and enters R2Q as is)."""
    mo = Uniform_Topology(60, 0.4, 0.2, 0.1, "uniform", seed=16)
    Rij = mo.RijMat.copy()
    Rij[:, :, [5, 40, 200]] *= 1.03
    e = int(np.argmax(np.einsum("aak->k", Rij)))                             # a small angle: trace + 1 stays positive after the stretch
    Rij[:, :, e] = Rij[:, :, e] @ np.diag([1.6, 1.0, 1.0])
    R, info, tr = check(Rij, mo.Ind, mode)
    assert info["warned_edges"] == 3
    R_plain, info_plain = FN[mode](mo.RijMat, mo.Ind, return_info=True)
    assert info_plain["warned_edges"] == 0 and not np.array_equal(info["R_l1"], info_plain["R_l1"])


def test_component_tie_goes_to_the_smallest_node_id():
    """Two 15-node pieces on ids 2-16 and 21-35 (ids 1 and 17-20 untouched), the second piece's rows listed first: the piece that
    holds node 2 is solved."""
    a = Uniform_Topology(15, 0.6, 0.1, 0.05, "uniform", seed=20)
    b = Uniform_Topology(15, 0.6, 0.1, 0.05, "uniform", seed=21)
    Ind = np.concatenate([b.Ind + 20, a.Ind + 1])
    Rij = np.concatenate([b.RijMat, a.RijMat], axis=2)
    for mode in ("GM", "L12"):
        R, info, tr = check(Rij, Ind, mode)
        assert info["comp_nodes"] == 15 and info["comp_edges"] == a.Ind.shape[0]
        keep = np.zeros(35, dtype=bool); keep[1:16] = True
        assert not np.isnan(R[:, :, keep]).any() and np.isnan(R[:, :, ~keep]).all()


def test_disconnected_graph_nan_placement():
    """Two pieces (20 and 12 nodes) and the node ids 21-25 that no edge touches: the 20-node piece is solved, the rest is NaN."""
    rng = np.random.default_rng(5)
    a = Uniform_Topology(20, 0.5, 0.1, 0.05, "uniform", seed=6)
    b = Uniform_Topology(12, 0.6, 0.1, 0.05, "uniform", seed=7)
    Ind = np.concatenate([a.Ind, b.Ind + 25])
    Rij = np.concatenate([a.RijMat, b.RijMat], axis=2)
    order = rng.permutation(Ind.shape[0])
    Ind, Rij = Ind[order], Rij[:, :, order]
    Rinit = random_rotations(37, rng)
    for mode in ("GM", "L12"):
        R, info, tr = check(Rij, Ind, mode)
        assert R.shape[2] == 37 and info["comp_nodes"] == 20
        assert np.isnan(R[:, :, 20:]).all() and not np.isnan(R[:, :, :20]).any()
    R, info, _ = check(Rij, Ind, "GM", Rinit=Rinit)                       # the component's rows of Rinit
    assert np.isnan(R[:, :, 20:]).all()


@pytest.mark.parametrize("mode", ["GM", "L12"])
def test_unsorted_ind_follows_the_caller_row_order(mode):
    mo = Uniform_Topology(60, 0.4, 0.2, 0.1, "uniform", seed=8)
    perm = np.random.default_rng(9).permutation(mo.Ind.shape[0])
    Ind, Rij = mo.Ind[perm], mo.RijMat[:, :, perm]
    R, info, tr = check(Rij, Ind, mode)
    R_sorted = FN[mode](mo.RijMat, mo.Ind)
    assert not np.array_equal(R, R_sorted) or tr["tree_passes"] == 1       # another tree: another start (unless both coincide)


def test_rinit_sigma_and_max_iterations():
    mo = Uniform_Topology(50, 0.4, 0.2, 0.1, "uniform", seed=10)
    Rinit = random_rotations(50, np.random.default_rng(11))
    check(mo.RijMat, mo.Ind, "GM", Rinit=Rinit)
    check(mo.RijMat, mo.Ind, "GM", SIGMA=2.0)
    R, info, tr = check(mo.RijMat, mo.Ind, "L12", MaxIterations=[1, 1])
    assert info["l1_iters"] == 1 and info["irls_iters"] == 1


def test_det_negative_edge_raises_with_its_row():
    mo = Uniform_Topology(30, 0.5, 0.1, 0.05, "uniform", seed=12)
    Rij = mo.RijMat.copy()
    Rij[:, :, 7] = -Rij[:, :, 7]
    Rij[:, :, 11] = -Rij[:, :, 11]
    with pytest.raises(_lib.DescError, match=r"det\(RR\(:,:,8\)\)"):
        IRLS_GM(Rij, mo.Ind)
    perm = np.arange(mo.Ind.shape[0])[::-1]
    with pytest.raises(_lib.DescError, match=r"det\(RR\(:,:,%d\)\)" % (mo.Ind.shape[0] - 11)):
        IRLS_GM(Rij[:, :, perm], mo.Ind[perm])
    Rij = mo.RijMat.copy()
    Rij[:, :, 3] = Rij[:, :, 3] * 1.2
    with pytest.raises(_lib.DescError, match=r"svd\(RR\(:,:,4\)\)"):
        IRLS_L12(Rij, mo.Ind)


def test_two_runs_are_bitwise_equal():
    mo = Nonuniform_Topology(120, 0.4, 0.3, 0.5, 0.1, 0.2, "adv", seed=13)
    for fn in (IRLS_GM, IRLS_L12):
        a, ia = fn(mo.RijMat, mo.Ind, return_info=True)
        b, ib = fn(mo.RijMat, mo.Ind, return_info=True)
        assert np.array_equal(a, b) and np.array_equal(ia["R_l1"], ib["R_l1"]) and ia["cg_iters_l1"] == ib["cg_iters_l1"]


# ---- full size and demo --------------------------------------------------------------------------------------------------------
def test_c2_against_oracle():
    sys.path.insert(0, ROOT)
    import bench
    mo = bench.generate("C2")[0]
    check(mo.RijMat, mo.Ind, "GM")


@pytest.mark.parametrize("mode", ["GM", "L12"])
def test_c4(mode):
    sys.path.insert(0, ROOT)
    import bench
    mo = bench.generate("C4")[0]
    R, info = FN[mode](mo.RijMat, mo.Ind, return_info=True)
    for X in (R, info["R_l1"]):
        Rt = np.einsum("abk,cbk->kac", X, X)
        assert np.abs(Rt - np.eye(3)).max() < 1e-6
        assert np.abs(np.linalg.det(np.transpose(X, (2, 0, 1))) - 1).max() < 1e-6
    assert info["cg_unconverged"] == 0
    R2, info2 = FN[mode](mo.RijMat, mo.Ind, return_info=True)
    assert np.array_equal(R, R2)
    _, _, mean_err, median_err = Rotation_Alignment(R, mo.R_orig)
    assert np.isfinite(mean_err) and np.isfinite(median_err)


def test_demo_eight_rows():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import compare_algorithms
    rows, _ = compare_algorithms.run(verbose=False, full=True, irls=True)
    assert [r[0] for r in rows] == ["Spectral", "IRLS-GM", "IRLS-L0.5", "CEMP+MST", "CEMP+GCW", "MPLS", "DESC_init", "DESC"]
    assert all(np.isfinite(r[1]) and np.isfinite(r[2]) for r in rows)

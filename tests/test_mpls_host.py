"""MPLS (Algorithms/MPLS.m) without a GPU: known answers of the NumPy restatement (tests/mpls_oracle.py) and the loud refusal of
the device entry points when no GPU is visible."""
import numpy as np
import pytest

from desc_amd import _lib
from desc_amd.models import Uniform_Topology
from tests.mpls_oracle import cemp_stage, h_step, kruskal, mpls_oracle, propagate

DEMO_CEMP = dict(max_iter=6, reweighting=[2.0 ** k for k in range(6)], nsample=20)
DEMO_MPLS = dict(stop_threshold=1e-3, max_iter=100, reweighting=[32.0], thresholding=[0.95, 0.9, 0.85, 0.8],
                 cycle_info_ratio=1.0 / (np.arange(1, 101) + 1))


def test_edge_without_cycles_gets_h_two_thirds():
    """MPLS.m:239 leaves HVec(~IndPosbin) alone: a zero cycle product gives S0 = |acos(-1/2)|/pi and weights 1/nsample."""
    Ind = np.array([[1, 2], [1, 3], [2, 3], [3, 4]])                    # (3, 4) is a pendant edge
    R = np.repeat(np.eye(3)[:, :, None], 4, axis=2)
    st = cemp_stage(Ind, R, 3, [1.0], 7)
    assert list(st["IndPosbin"]) == [True, True, True, False]
    assert st["SVec"][3] == 1.0
    H = h_step(st, np.array([0.3, 0.1, 0.2, 0.5]), 5.0)
    assert abs(H[3] - 2.0 / 3.0) < 1e-15
    assert np.all(np.abs(st["S0Mat"][:, 3] - 2.0 / 3.0) < 1e-15)


def test_complete_graph_of_identities_gives_the_star_and_identity():
    """Every cycle is consistent: S = 0 everywhere, all keys tie at 1.0, and the index order picks the edges (1, j)."""
    n = 7
    Ind = np.array([(i, j) for i in range(1, n + 1) for j in range(i + 1, n + 1)])
    R = np.repeat(np.eye(3)[:, :, None], Ind.shape[0], axis=2)
    st = cemp_stage(Ind, R, 4, [1.0, 2.0], 10)
    assert np.all(st["SVec"] == 0.0)
    tree = kruskal(Ind, st["SVec"])
    assert [tuple(Ind[e]) for e in tree] == [(1, j) for j in range(2, n + 1)]
    assert np.array_equal(propagate(Ind, R, tree), np.repeat(np.eye(3)[:, :, None], n, axis=2))


def test_oracle_tree_weight_equals_scipy():
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    rng = np.random.default_rng(3)
    mo = Uniform_Topology(60, 0.3, 0.2, 0.1, "uniform", seed=3)
    S = rng.random(mo.Ind.shape[0])
    tree = kruskal(mo.Ind, S)
    G = sp.coo_matrix((S + 1.0, (mo.Ind[:, 1] - 1, mo.Ind[:, 0] - 1)), shape=(60, 60)).tocsr()     # MPLS.m:162
    ref = csgraph.minimum_spanning_tree(G).sum()
    assert tree is not None and len(tree) == 59
    assert abs((S[tree] + 1.0).sum() - ref) < 1e-9


def test_oracle_disconnected_graph_has_no_tree():
    Ind = np.array([[1, 2], [3, 4]])
    assert kruskal(Ind, np.zeros(2)) is None


def test_oracle_runs_the_demo_loop():
    mo = Uniform_Topology(40, 0.5, 0.2, 0.1, "uniform", seed=1)
    out = mpls_oracle(mo.Ind, mo.RijMat, DEMO_CEMP, DEMO_MPLS, seed=1)
    assert 1 <= out["iters"] < 100 and out["score"] <= 1e-3
    Rt = np.einsum("abk,cbk->kac", out["R_est"], out["R_est"])
    assert np.abs(Rt - np.eye(3)).max() < 1e-12


def test_no_gpu_mpls_mst_cemp_gcw_fail_loudly():
    if _lib.load().desc_device_count() > 0:
        pytest.skip("a GPU is visible")
    from desc_amd import CEMP_GCW, MPLS, MST
    mo = Uniform_Topology(20, 0.5, 0.2, 0.1, "uniform", seed=1)
    for call in (lambda: MPLS(mo.Ind, mo.RijMat, DEMO_CEMP, DEMO_MPLS), lambda: MST(mo.Ind, mo.RijMat, np.zeros(mo.Ind.shape[0])),
                 lambda: CEMP_GCW(mo.Ind, mo.RijMat, DEMO_CEMP)):
        with pytest.raises(_lib.DescError):
            call()

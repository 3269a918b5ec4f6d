"""GPU parity of MPLS (Algorithms/MPLS.m:31-257), its MST step (:160-193) and CEMP_GCW against the NumPy restatements
(tests/mpls_oracle.py, oracle/spectral_oracle.py).  Tolerances: SVec 1e-12 (as CEMP), R_init 1e-10 (3x3 products along the tree),
R_est 1e-7 (PCG vs lstsq through hard quantile thresholds, as the refinement test)."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg

from desc_amd import CEMP, CEMP_GCW, MPLS, MST, Rotation_Alignment, Spectral, _lib
from desc_amd.models import Uniform_Topology
from oracle.refine_oracle import R2Q, q2R
from oracle.spectral_oracle import _blk, _project
from tests.mpls_oracle import cemp_stage, kruskal, mpls_oracle, propagate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def demo_params(nsample, seed):
    """Demo/compare_algorithms.m:26-36."""
    cemp = dict(max_iter=6, reweighting=[2.0 ** k for k in range(6)], nsample=nsample, seed=seed)
    mpls = dict(stop_threshold=1e-3, max_iter=100, reweighting=cemp["reweighting"][-1], thresholding=[0.95, 0.9, 0.85, 0.8],
                cycle_info_ratio=1.0 / (np.arange(1, 101) + 1))
    return cemp, mpls


def random_rotations(k, rng):
    Q = np.linalg.qr(rng.standard_normal((k, 3, 3)))[0]
    Q[np.linalg.det(Q) < 0, :, 0] *= -1
    return np.ascontiguousarray(np.transpose(Q, (1, 2, 0)))


def check_against_oracle(Ind, RijMat, cemp, mpls, seed):
    R_est, R_init, info = MPLS(Ind, RijMat, cemp, mpls, return_info=True)
    S = info["SVec"]
    st = cemp_stage(Ind, RijMat, cemp["max_iter"], cemp["reweighting"], cemp["nsample"], seed)
    assert np.abs(S - st["SVec"]).max() < 1e-12
    ref = mpls_oracle(Ind, RijMat, cemp, mpls, seed=seed, svec_for_tree=S)
    assert np.abs(R_init - ref["R_init"]).max() < 1e-10
    assert info["iters"] == ref["iters"], (info["iters"], ref["iters"])
    assert np.abs(R_est - ref["R_est"]).max() < 1e-7, np.abs(R_est - ref["R_est"]).max()
    assert abs(info["score"] - ref["score"]) < 1e-9
    return R_est, R_init, info, ref


# ---- MST ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["random", "quantised", "zero", "near_one"])
def test_mst_tree_equals_kruskal(case):
    rng = np.random.default_rng(7)
    mo = Uniform_Topology(90, 0.3, 0.2, 0.1, "uniform", seed=5)
    m = mo.Ind.shape[0]
    S = {"random": rng.random(m), "quantised": np.round(rng.random(m) * 3) / 3, "zero": np.zeros(m),
         "near_one": 1e-17 * rng.integers(0, 4, m)}[case]                   # fl(S + 1) merges all of these into 1.0
    R, info = MST(mo.Ind, mo.RijMat, S, return_info=True)
    tree = kruskal(mo.Ind, S)
    assert np.array_equal(info["tree_edges"], tree)
    assert np.abs(R - propagate(mo.Ind, mo.RijMat, tree)).max() < 1e-12


def test_mst_complete_graph_of_identities_is_the_star():
    n = 12
    Ind = np.array([(i, j) for i in range(1, n + 1) for j in range(i + 1, n + 1)])
    R0 = np.repeat(np.eye(3)[:, :, None], Ind.shape[0], axis=2)
    S = CEMP(Ind, R0, dict(max_iter=3, reweighting=[1.0], nsample=10))
    assert np.all(S == 0.0)
    R, info = MST(Ind, R0, S, return_info=True)
    assert [tuple(Ind[e]) for e in info["tree_edges"]] == [(1, j) for j in range(2, n + 1)]
    assert np.array_equal(R, np.repeat(np.eye(3)[:, :, None], n, axis=2))


# ---- MPLS vs the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,q,seed,nsample", [(40, 0.5, 0.2, 1, 20), (70, 0.4, 0.3, 2, 50), (100, 0.3, 0.2, 3, 80), (60, 0.6, 0.1, 4, 100)])
def test_mpls_matches_oracle(n, p, q, seed, nsample):
    mo = Uniform_Topology(n, p, q, 0.1, "uniform", seed=seed)
    cemp, mpls = demo_params(nsample, seed)
    R_est, R_init, info, ref = check_against_oracle(mo.Ind, mo.RijMat, cemp, mpls, seed)
    assert info["cg_unconverged"] == 0
    assert abs(Rotation_Alignment(R_est, mo.R_orig)[2] - Rotation_Alignment(ref["R_est"], mo.R_orig)[2]) < 1e-6


def test_pendant_edges_take_the_two_thirds_rule():
    """Edges without a 3-cycle: H = 2/3 (MPLS.m:239 is commented out), against the oracle."""
    rng = np.random.default_rng(11)
    mo = Uniform_Topology(50, 0.3, 0.2, 0.1, "uniform", seed=11)
    extra = np.array([[int(rng.integers(1, 51)), 50 + t] for t in range(1, 7)])          # six pendant nodes 51..56
    Ind = np.vstack([mo.Ind, extra])
    RijMat = np.concatenate([mo.RijMat, random_rotations(6, rng)], axis=2)
    order = np.lexsort((Ind[:, 1], Ind[:, 0]))            # the keyed samples follow the (i, j)-sorted edge index: hand the oracle that order
    Ind, RijMat = Ind[order], RijMat[:, :, order]
    cemp, mpls = demo_params(30, 2)
    R_est, R_init, info, ref = check_against_oracle(Ind, RijMat, cemp, mpls, 2)
    assert info["m_pos"] < Ind.shape[0]
    assert np.sum(~ref["state"]["IndPosbin"]) >= 6


def test_short_parameter_vectors_are_padded():
    mo = Uniform_Topology(45, 0.5, 0.25, 0.1, "uniform", seed=6)
    cemp = dict(max_iter=5, reweighting=[1.0, 2.0], nsample=25, seed=6)
    mpls = dict(stop_threshold=1e-4, max_iter=30, reweighting=[4.0, 8.0], thresholding=[0.9], cycle_info_ratio=[0.5, 0.25])
    check_against_oracle(mo.Ind, mo.RijMat, cemp, mpls, 6)


def test_max_iter_one_returns_the_initialisation():
    mo = Uniform_Topology(40, 0.5, 0.2, 0.1, "uniform", seed=8)
    cemp, mpls = demo_params(20, 8)
    R_est, R_init, info = MPLS(mo.Ind, mo.RijMat, cemp, dict(mpls, max_iter=1), return_info=True)
    assert info["iters"] == 0
    Q = R2Q(R_init)
    ref = np.stack([q2R(Q[i]) for i in range(Q.shape[0])], axis=2)
    assert np.abs(R_est - ref).max() < 1e-12


def test_stop_on_threshold_before_max_iter():
    mo = Uniform_Topology(50, 0.5, 0.2, 0.1, "uniform", seed=9)
    cemp, mpls = demo_params(30, 9)
    R_est, R_init, info, ref = check_against_oracle(mo.Ind, mo.RijMat, cemp, dict(mpls, stop_threshold=2e-2), 9)
    assert 1 <= info["iters"] < 99 and info["score"] <= 2e-2


def test_triangle():
    rng = np.random.default_rng(3)
    Ind = np.array([[1, 2], [1, 3], [2, 3]])
    RijMat = random_rotations(3, rng)
    cemp, mpls = demo_params(10, 0)
    check_against_oracle(Ind, RijMat, cemp, mpls, 0)


# ---- composition, paths, inputs ----------------------------------------------------------------------------------------------
def test_r_init_is_mst_of_cemp():
    mo = Uniform_Topology(80, 0.4, 0.3, 0.1, "uniform", seed=12)
    cemp, mpls = demo_params(50, 12)
    R_est, R_init = MPLS(mo.Ind, mo.RijMat, cemp, mpls)
    S = CEMP(mo.Ind, mo.RijMat, cemp)
    assert np.array_equal(R_init, MST(mo.Ind, mo.RijMat, S))


@pytest.mark.parametrize("nsample", [50, 90])
def test_h_step_tile_path_equals_plain_path(nsample, monkeypatch):
    mo = Uniform_Topology(260, 0.5, 0.2, 0.1, "uniform", seed=9)
    cemp, mpls = demo_params(nsample, 5)
    monkeypatch.setenv("DESC_DEBUG_CEMP_TILES", "0")
    plain = MPLS(mo.Ind, mo.RijMat, cemp, mpls, return_info=True)
    monkeypatch.setenv("DESC_DEBUG_CEMP_TILES", "1")
    for bi, jb in ((1, 32), (7, 50), (16, 40)):
        monkeypatch.setenv("DESC_DEBUG_CEMP_BI", str(bi))
        monkeypatch.setenv("DESC_DEBUG_CEMP_JB", str(jb))
        tiles = MPLS(mo.Ind, mo.RijMat, cemp, mpls, return_info=True)
        assert np.array_equal(plain[2]["SVec"], tiles[2]["SVec"])
        assert np.array_equal(plain[1], tiles[1]) and np.array_equal(plain[0], tiles[0])
        assert plain[2]["iters"] == tiles[2]["iters"]


def test_permuted_double_fortran_inputs_equal_sorted():
    mo = Uniform_Topology(60, 0.5, 0.2, 0.1, "uniform", seed=13)
    cemp, mpls = demo_params(30, 13)
    R_est, R_init = MPLS(mo.Ind, mo.RijMat, cemp, mpls)
    perm = np.random.default_rng(1).permutation(mo.Ind.shape[0])
    Ind_p = mo.Ind[perm].astype(np.float64)
    R_p = np.asfortranarray(mo.RijMat[:, :, perm])
    R_est2, R_init2 = MPLS(Ind_p, R_p, cemp, mpls)
    assert np.array_equal(R_est, R_est2) and np.array_equal(R_init, R_init2)
    S = CEMP(mo.Ind, mo.RijMat, cemp)
    _, info = MST(mo.Ind, mo.RijMat, S, return_info=True)
    _, info_p = MST(Ind_p, R_p, S[perm], return_info=True)
    assert np.array_equal(np.sort(perm[info_p["tree_edges"]]), info["tree_edges"])


def test_disconnected_input_is_refused():
    rng = np.random.default_rng(4)
    Ind = np.array([[1, 2], [1, 3], [2, 3], [4, 5], [4, 6], [5, 6]])                      # two triangles
    RijMat = random_rotations(6, rng)
    cemp, mpls = demo_params(10, 0)
    with pytest.raises(_lib.DescError, match="2 components"):
        MPLS(Ind, RijMat, cemp, mpls)
    with pytest.raises(_lib.DescError, match="2 components"):
        MST(Ind, RijMat, np.zeros(6))
    Ind_gap = np.array([[1, 2], [1, 3], [2, 3], [3, 5]])                                  # node 4 touches no edge
    with pytest.raises((_lib.DescError, ValueError)):
        MPLS(Ind_gap, random_rotations(4, rng), cemp, mpls)
    with pytest.raises((_lib.DescError, ValueError)):
        MST(Ind_gap, random_rotations(4, rng), np.zeros(4))


def test_cemp_gcw_matches_dense_oracle():
    """CEMP_GCW.m:137-160: weights 1/(SVec + 1e-8), row-normalised, top-3 eigenvectors, per-node projection."""
    mo = Uniform_Topology(70, 0.5, 0.2, 0.1, "uniform", seed=3)
    cemp = dict(max_iter=6, reweighting=[2.0 ** k for k in range(6)], nsample=50, seed=3)
    R = CEMP_GCW(mo.Ind, mo.RijMat, cemp)
    S = CEMP(mo.Ind, mo.RijMat, cemp)
    n = 70
    B = _blk(mo.Ind, mo.RijMat, n)
    A = np.zeros((n, n)); Sm = np.zeros((n, n))
    A[mo.Ind[:, 0] - 1, mo.Ind[:, 1] - 1] = 1; A = A + A.T
    Sm[mo.Ind[:, 0] - 1, mo.Ind[:, 1] - 1] = S; Sm = Sm + Sm.T
    W = (1.0 / (Sm + 1e-8)) * A
    W = np.diag(1.0 / W.sum(axis=1)) @ W
    lam, vec = scipy.linalg.eig(B * np.kron(W, np.ones((3, 3))))
    V = np.real(vec[:, np.argsort(-lam.real)[:3]])
    ref = _project(V / np.linalg.norm(V, axis=0), n)
    R_al = Rotation_Alignment(R, ref)[0]
    assert np.abs(R_al - ref).max() < 1e-7


# ---- full size and demo --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C2", "C4"])
def test_fullsize_mpls(name):
    sys.path.insert(0, ROOT)
    import bench
    mo = bench.generate(name)[0]
    cemp, mpls = demo_params(50, 0)
    R_est, R_init, info = MPLS(mo.Ind, mo.RijMat, cemp, mpls, return_info=True)
    # R_init: 3x3 products along the tree.  R_est keeps the reference's arithmetic: R2Q.m divides by cos(theta/2), so a node whose
    # R_init turns by nearly pi gets a quaternion whose norm is off by ~1e-16 / (pi - theta)^2; Weighted_LAA never renormalises Q and
    # q2R.m turns that into an orthogonality defect once the node's angle has moved (1.8e-10 at C2, 1.5e-8 at C4 measured)
    for R, tol in ((R_init, 1e-12), (R_est, 1e-6)):
        Rt = np.einsum("abk,cbk->kac", R, R)
        assert np.abs(Rt - np.eye(3)).max() < tol
        assert np.abs(np.linalg.det(np.transpose(R, (2, 0, 1))) - 1).max() < tol
    assert info["cg_unconverged"] == 0
    R_est2, R_init2, info2 = MPLS(mo.Ind, mo.RijMat, cemp, mpls, return_info=True)
    assert np.array_equal(R_est, R_est2) and np.array_equal(R_init, R_init2) and info["iters"] == info2["iters"]
    if name == "C2":
        _, tinfo = MST(mo.Ind, mo.RijMat, info["SVec"], return_info=True)
        assert np.array_equal(tinfo["tree_edges"], kruskal(mo.Ind, info["SVec"]))
    e_mpls = Rotation_Alignment(R_est, mo.R_orig)[2]
    e_mst = Rotation_Alignment(R_init, mo.R_orig)[2]
    e_sp = Rotation_Alignment(Spectral(mo.Ind, mo.RijMat), mo.R_orig)[2]
    assert e_mpls <= e_mst + 0.05 and e_mpls < 0.5 * e_sp, (e_mpls, e_mst, e_sp)


def test_demo_full_table():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import compare_algorithms
    rows, _ = compare_algorithms.run(verbose=False, full=True)
    names = [r[0] for r in rows]
    assert names == ["Spectral", "CEMP+MST", "CEMP+GCW", "MPLS", "DESC_init", "DESC"]
    err = dict((r[0], r[1]) for r in rows)
    assert err["MPLS"] < err["Spectral"]

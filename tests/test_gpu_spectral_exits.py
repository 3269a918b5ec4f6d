"""The exits of the Spectral / GCW eigen-solve (desc_amd/csrc/spectral.hip: spectral_impl): what it reports in info, the max_iters
exit with its closing Rayleigh-Ritz, m = 0, n = 1, a node without edges under row normalisation, and the errors.  Graphs of n <= 150.

The eigenvalue tolerance is the residual bound of a symmetric matrix -- a Ritz pair with residual r has an eigenvalue within |r| of
theta; tests/test_spectral_host.py checks the gap lambda_3 - lambda_4 > 1e-3 scale that makes it lambda_c -- plus the summation bound
of the Gram reductions over 3n rows:  |theta_c - lambda_c| <= (info["residual"] + 4 * 3n * eps) * scale,  scale = max(|lambda_1|, sigma)
(info["residual"] is relative to that scale)."""
import numpy as np
import pytest

from desc_amd import _lib as lib
from oracle.spectral_oracle import gcw_oracle, rotation_alignment, spectral_oracle
from tests import spectral_cases as K
from tests import spectral_kernels_oracle as O

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TOL = 1e-12


def _prob(n, ii, jj, rij):
    return lib.ProblemArrays(n, ii, jj, np.ascontiguousarray(np.asarray(rij, dtype=np.float64).reshape(-1)))


def _run(name, **kw):
    w, S, norm = K.exit_inputs()[name]
    _, n, ii, jj, rij = K.exit_problem()
    if S is not None:
        dp = lib.DeviceProblem(_prob(n, ii, jj, rij), 0)
        try:
            return lib.gcw_run(dp, S, **kw)
        finally:
            dp.free()
    return lib.spectral_run(_prob(n, ii, jj, rij), w, norm, **kw)


def _valid_rotations(R):
    return max(O.so3_defect(R[:, :, v]) for v in range(R.shape[2])) <= 16 * EPS       # what tests/test_spectral_host.py allows project_so3


def _eig_tol(info, n, scale):
    return (info["residual"] + 4 * 3 * n * EPS) * scale


@pytest.mark.parametrize("name", list(K.exit_inputs()))
def test_reported_eigenvalues_are_the_dense_matrix_s(name):
    A, sigma = K.exit_dense(name)
    lam = np.linalg.eigvalsh(A)[::-1]
    scale = max(abs(lam[0]), sigma)
    R, info = _run(name, tol=TOL)
    n = R.shape[2]
    assert info["converged"] and info["residual"] <= TOL and info["iters"] >= 1 and info["products"] >= info["iters"], info
    theta = np.array(info["eigenvalues"])
    assert (np.abs(theta - lam[:3]) <= _eig_tol(info, n, scale)).all(), (theta, lam[:3], info)
    assert _valid_rotations(R)


@pytest.mark.parametrize("tight,products", [(None, 10), ("0", 18)])
def test_max_iters_exit_takes_a_closing_rayleigh_ritz(tight, products, monkeypatch):
    """max_iters = 1: one Rayleigh-Ritz (1 product), not converged from the hashed start, one filter pass -- of degree CHEB_FIRST = 8
    under the tight scheme, CHEB_DEG = 16 under the fixed one --, then the loop is over and the new basis gets the Rayleigh-Ritz the
    returned vectors and eigenvalues belong to (1 product).  Ritz values of a symmetric matrix never exceed its eigenvalues."""
    monkeypatch.delenv("DESC_DEBUG_SPECTRAL_FIRST", raising=False)
    if tight is None:
        monkeypatch.delenv("DESC_DEBUG_SPECTRAL_TIGHT", raising=False)
    else:
        monkeypatch.setenv("DESC_DEBUG_SPECTRAL_TIGHT", tight)
    A, sigma = K.exit_dense("spectral")
    lam = np.linalg.eigvalsh(A)[::-1]
    R, info = _run("spectral", tol=TOL, max_iters=1)
    assert not info["converged"] and info["iters"] == 1 and info["products"] == products, info
    assert info["residual"] > TOL
    theta = np.array(info["eigenvalues"])
    assert (theta <= lam[:3] + _eig_tol(info, R.shape[2], max(abs(lam[0]), sigma))).all(), (theta, lam[:3])
    assert (np.diff(theta) <= 0).all()
    assert _valid_rotations(R)


@pytest.mark.parametrize("n", [2, 5])
def test_a_graph_without_edges(n):
    empty = np.zeros(0, dtype=np.int32)
    R, info = lib.spectral_run(_prob(n, empty, empty, np.zeros(0)), tol=TOL)
    assert info["converged"] and info["products"] == 1 and info["iters"] == 1 and info["eigenvalues"] == [0.0, 0.0, 0.0], info
    assert info["residual"] == 0.0
    assert _valid_rotations(R)


def test_one_node_gets_the_identity():
    empty = np.zeros(0, dtype=np.int32)
    for normalize in (False, True):
        R, info = lib.spectral_run(_prob(1, empty, empty, np.zeros(0)), None, normalize)
        assert np.array_equal(R[:, :, 0], np.eye(3))
        assert info["converged"] and info["iters"] == 0 and info["products"] == 0 and info["eigenvalues"] == [0.0, 0.0, 0.0] and info["residual"] == 0.0
    dp = lib.DeviceProblem(_prob(1, empty, empty, np.zeros(0)), 0)
    try:
        for R, info in (lib.spectral_run(dp), lib.gcw_run(dp, np.zeros(0))):
            assert np.array_equal(R[:, :, 0], np.eye(3)) and info["converged"] and info["iters"] == 0 and info["products"] == 0
    finally:
        dp.free()


def test_a_node_without_edges_under_row_normalisation():
    """Its degree is 0, so D^-1/2 gives it a zero block: identity.  NumPy's gcw_oracle divides by zero there; it runs on the graph
    without that node, and the other nodes must match it."""
    mo, n, ii, jj, rij = K.exit_problem()
    S = K.exit_inputs()["gcw"][1]
    dp = lib.DeviceProblem(_prob(n + 1, ii, jj, rij), 0)
    try:
        R, info = lib.gcw_run(dp, S, tol=TOL)
    finally:
        dp.free()
    assert info["converged"], info
    assert np.array_equal(R[:, :, n], np.eye(3))
    R_ref = gcw_oracle(mo.Ind, mo.RijMat, S)
    R_al = rotation_alignment(R[:, :, :n], R_ref)[0]
    assert np.abs(R_al - R_ref).max() < 1e-8
    assert _valid_rotations(R)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_a_bad_weight_is_refused_by_name(bad):
    _, n, ii, jj, rij = K.exit_problem()
    m = len(ii)
    for e in (0, m // 2, m - 1):
        w = np.ones(m); w[e] = bad
        with pytest.raises(lib.DescError) as ei:
            lib.spectral_run(_prob(n, ii, jj, rij), w, True)
        assert ei.value.code == lib.ERR_INVALID and ("weight %d " % e) in str(ei.value), str(ei.value)


@pytest.mark.parametrize("bad", [-1.0, float("nan")])
def test_a_bad_s_vec_entry_is_refused_by_node(bad):
    _, n, ii, jj, rij = K.exit_problem()
    m = len(ii)
    dp = lib.DeviceProblem(_prob(n, ii, jj, rij), 0)
    try:
        for e in (0, m // 2, m - 1):
            S = K.exit_inputs()["gcw"][1].copy(); S[e] = bad
            with pytest.raises(lib.DescError) as ei:
                lib.gcw_run(dp, S)
            v = int(min(ii[e], jj[e]))
            assert ei.value.code == lib.ERR_INVALID and ("negative or non-finite entry (node %d)" % v) in str(ei.value), str(ei.value)
    finally:
        dp.free()


def test_an_infinite_s_vec_entry_is_a_zero_weight():
    mo, n, ii, jj, rij = K.exit_problem()
    S = K.exit_inputs()["gcw"][1].copy()
    S[len(S) // 2] = np.inf
    dp = lib.DeviceProblem(_prob(n, ii, jj, rij), 0)
    try:
        R, info = lib.gcw_run(dp, S, tol=TOL)
    finally:
        dp.free()
    assert info["converged"], info
    R_ref = gcw_oracle(mo.Ind, mo.RijMat, S)                           # 1 / (inf + 1e-8) = 0 there as well
    assert np.abs(rotation_alignment(R, R_ref)[0] - R_ref).max() < 1e-8


def test_size_mismatches_never_reach_the_device():
    _, n, ii, jj, rij = K.exit_problem()
    m = len(ii)
    with pytest.raises(ValueError):
        lib.spectral_run(_prob(n, ii, jj, rij), np.ones(m + 1), True)
    dp = lib.DeviceProblem(_prob(n, ii, jj, rij), 0)
    try:
        with pytest.raises(ValueError):
            lib.gcw_run(dp, np.ones(m - 1))
        with pytest.raises(ValueError):
            lib.hook_spectral_row_wsum(dp, np.ones(m + 1))
        with pytest.raises(ValueError):
            lib.hook_spectral_spmm(dp, np.zeros(18 * m), np.zeros(3 * n * 6 - 1), np.zeros(3 * n * 6), 1.0, 0.0, 0.0)
    finally:
        dp.free()

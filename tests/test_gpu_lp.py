"""GPU tests of linprog_sij (Algorithms/linprog_sij.m) and DESC_init, through the public Python entry points.

The LP optimum is not unique, so S_vec is never compared with HiGHS's x* element by element: a solution is checked through its
certificates -- viol = max((Kx - b)+), P = sum x, D = -b'y + sum min(0, 1 + K'y) -- which are exact statements (every y >= 0 is dual
feasible, so D <= f* <= any feasible P; against HiGHS's dual y*, P >= f* - y*'(Kx - b)+).  The bounds below follow from the stopping rule
and duality; none of them is a measured number."""
import numpy as np
import pytest

from desc_amd import DESC, DESC_PGD, DESC_init, ConstantStepSize, Rotation_Alignment, linprog_sij
from desc_amd.models import Nonuniform_Topology, Uniform_Topology
from oracle.spectral_oracle import rotation_alignment
from tests import lp_oracle as O

pytestmark = pytest.mark.gpu

SEED = 3


def sparse_model():
    """A sparse graph in which some edges lie on no triangle."""
    return Uniform_Topology(60, 0.08, 0.2, 0.05, "uniform", seed=5)


GRAPHS = {
    "n30-q0.2": lambda: Uniform_Topology(30, 0.5, 0.2, 0.05, "uniform", seed=3),
    "n30-q0.3": lambda: Uniform_Topology(30, 0.5, 0.3, 0.05, "uniform", seed=3),
    "n60-q0.2": lambda: Uniform_Topology(60, 0.5, 0.2, 0.05, "uniform", seed=3),
    "n60-q0.3": lambda: Uniform_Topology(60, 0.5, 0.3, 0.05, "uniform", seed=3),
    "nonuniform70": lambda: Nonuniform_Topology(70, 0.5, 0.4, 0.5, 0.1, 0.1, "adv", seed=104),
    "sparse": sparse_model,
}
_cache = {}


def problem(name):
    if name not in _cache:
        mo = GRAPHS[name]()
        _cache[name] = (mo,) + O.build_lp(mo.Ind, mo.RijMat, SEED)
    return _cache[name]


def in_so3(R):
    Rm = np.transpose(R, (2, 0, 1))
    return np.abs(Rm @ np.transpose(Rm, (0, 2, 1)) - np.eye(3)).max() < 1e-10 and np.abs(np.linalg.det(Rm) - 1).max() < 1e-10


@pytest.mark.parametrize("name", list(GRAPHS))
def test_structure_matches_the_restatement(name):
    mo, K, b, pos, k, ns = problem(name)
    Rest, S, info = linprog_sij(mo.Ind, mo.RijMat, dict(seed=SEED, max_iter=1), return_info=True)
    assert info["lp"]["nsample"] == ns and info["lp"]["m_pos"] == pos.size and info["lp"]["rows"] == K.shape[0]
    assert np.array_equal(info["pos_edges"], pos)
    assert np.array_equal(info["k"], k)
    nopos = np.setdiff1d(np.arange(mo.Ind.shape[0]), pos)
    if name == "sparse":
        assert nopos.size > 0 and pos.size > 0
    assert np.all(S[nopos] == 1.0)


def test_nsample_override():
    mo = GRAPHS["n30-q0.2"]()
    K, b, pos, k, ns = O.build_lp(mo.Ind, mo.RijMat, SEED, nsample=7)
    _, _, info = linprog_sij(mo.Ind, mo.RijMat, dict(seed=SEED, max_iter=1, nsample=7), return_info=True)
    assert info["lp"]["nsample"] == 7 and np.array_equal(info["k"], k)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_certificates(name):
    mo, K, b, pos, k, ns = problem(name)
    tol = 1e-5
    Rest, S, info = linprog_sij(mo.Ind, mo.RijMat, dict(seed=SEED, tol=tol, return_dual=True), return_info=True)
    lp = info["lp"]
    x, y = S[pos], info["y"].reshape(-1)
    f, xs, ys = O.solve_highs(K, b)
    viol, P, D = O.certificates(K, b, x, y)
    print("%s: iters %d restarts %d  viol %.3e  P %.12g  D %.12g  f* %.12g  loop %.1f ms" % (name, lp["iters"], lp["restarts"], viol, P, D, f, lp["ms_loop"]))
    assert lp["converged"] == 1
    assert viol <= tol
    assert P - D <= tol * (1 + abs(P) + abs(D))
    assert np.all(y >= 0) and np.all(S >= 0) and np.all(S <= 1)
    assert D <= f + 1e-9 * (1 + f)
    v = np.maximum(K @ x - b, 0.0)
    assert f - ys @ v - 1e-9 * (1 + f) <= P <= f + tol * (1 + abs(P) + abs(D))
    for got, ref in ((lp["viol"], viol), (lp["pobj"], P), (lp["dobj"], D)):          # 1e-9 relative (+ 1e-15: a violation is a difference of O(1) doubles)
        assert abs(got - ref) <= 1e-9 * abs(ref) + 1e-15, (got, ref)


@pytest.mark.parametrize("name", ["n30-q0.2", "n60-q0.3", "sparse"])
def test_kernels_follow_the_plain_recurrence(name):
    """restart = 0, tol = 0: exactly N plain steps.  Same arithmetic as tests/lp_oracle.py's pdhg_plain; only the order inside the fixed-order
    sums of K'y and of the edge's own term differs (and the last place of S0Mat's acos).  Measured on an MI355X: at most 2.1e-15 in x and
    2.1e-13 in y over these nine cases."""
    mo, K, b, pos, k, ns = problem(name)
    tau, sigma = O.step_sizes(K)
    for N in (1, 2, 50):
        _, S, info = linprog_sij(mo.Ind, mo.RijMat, dict(seed=SEED, tol=0.0, restart=0, max_iter=N, return_dual=True), return_info=True)
        x, y = O.pdhg_plain(K, b, tau, sigma, N)
        dx, dy = np.abs(S[pos] - x).max(), np.abs(info["y"].reshape(-1) - y).max()
        print("%s N %d: max|x - x_ref| %.3e  max|y - y_ref| %.3e" % (name, N, dx, dy))
        assert info["lp"]["iters"] == N and info["lp"]["converged"] == 0 and info["lp"]["restarts"] == 0
        assert dx <= 1e-12 and dy <= 1e-12


def test_two_runs_give_the_same_bits_and_rows_may_be_permuted():
    mo = GRAPHS["n60-q0.3"]()
    prm = dict(seed=SEED, tol=1e-4, return_dual=True)
    R1, S1, i1 = linprog_sij(mo.Ind, mo.RijMat, prm, return_info=True)
    R2, S2, i2 = linprog_sij(mo.Ind, mo.RijMat, prm, return_info=True)
    assert i1["lp"]["converged"] == 1 and i1["lp"]["restarts"] > 0
    assert np.array_equal(S1, S2) and np.array_equal(i1["y"], i2["y"]) and np.array_equal(R1, R2)
    perm = np.random.default_rng(0).permutation(mo.Ind.shape[0])
    R3, S3, i3 = linprog_sij(mo.Ind[perm], mo.RijMat[:, :, perm], prm, return_info=True)
    assert np.array_equal(S3, S1[perm]) and np.array_equal(R3, R1)
    assert np.array_equal(i3["pos_edges"], np.argsort(perm)[i1["pos_edges"]])


def test_iteration_cap_is_no_error(capfd):
    mo = GRAPHS["n60-q0.2"]()
    Rest, S, info = linprog_sij(mo.Ind, mo.RijMat, dict(seed=SEED, max_iter=10), return_info=True)
    assert info["lp"]["converged"] == 0 and info["lp"]["iters"] == 10
    assert np.all(S >= 0) and np.all(S <= 1)
    assert in_so3(info["R_gcw"]) and in_so3(Rest)
    assert "max_iter" in capfd.readouterr().err


@pytest.mark.parametrize("name", ["n30-q0.3", "n60-q0.2", "nonuniform70"])
def test_tail_matches_the_dense_restatement(name):
    """The device's own S_vec through lp_oracle.tail: tolerances of tests/test_gpu_spectral.py (1e-8 after alignment) and
    tests/test_gpu_refine.py (1e-7 on the rotation entries)."""
    mo = GRAPHS[name]()
    Rest, S, info = linprog_sij(mo.Ind, mo.RijMat, dict(seed=SEED), return_info=True)
    assert info["refine"]["cg_unconverged"] == 0 and info["spectral"]["converged"]
    R_gcw_ref, Rest_ref = O.tail(mo.Ind, mo.RijMat, S)
    d_gcw = np.abs(rotation_alignment(info["R_gcw"], R_gcw_ref)[0] - R_gcw_ref).max()
    d_est = np.abs(rotation_alignment(Rest, Rest_ref)[0] - Rest_ref).max()
    print("%s: aligned max|R_gcw - ref| %.3e  max|Rest - ref| %.3e  refine iters %d" % (name, d_gcw, d_est, info["refine"]["iters"]))
    assert d_gcw < 1e-8
    assert d_est < 1e-7


def test_desc_init_is_the_head_of_desc():
    mo = Uniform_Topology(80, 0.5, 0.2, 0.1, "uniform", seed=4)
    def prm(**kw):
        return dict(iters=40, learning_rate=0.01, Gradient=ConstantStepSize(0.01), verbose=False, seed=2, **kw)
    R_est, R_init, S_vec = DESC(mo.Ind, mo.RijMat, prm())
    R0, S0 = DESC_init(mo.Ind, mo.RijMat, prm())
    assert np.array_equal(R0, R_init) and np.array_equal(S0, S_vec)
    plots = dict(make_plots=True, ErrVec=mo.ErrVec, R_orig=mo.R_orig)
    R1, S1, info = DESC_init(mo.Ind, mo.RijMat, prm(**plots), return_info=True)
    S2, ref = DESC_PGD(mo.Ind, mo.RijMat, prm(**plots), return_info=True)
    assert np.array_equal(S1, S2)
    for key in ("svec_errors", "MSE_means", "MSE_medians", "obj"):
        assert np.array_equal(info["pgd"][key], ref[key]), key


def test_desc_init_appends_the_csv_rows_only_on_request(tmp_path):
    mo = Uniform_Topology(40, 0.5, 0.2, 0.1, "uniform", seed=4)
    prm = dict(iters=5, Gradient=ConstantStepSize(0.01), verbose=False, make_plots=True, ErrVec=mo.ErrVec, R_orig=mo.R_orig)
    DESC_init(mo.Ind, mo.RijMat, prm)
    assert list(tmp_path.iterdir()) == []
    DESC_init(mo.Ind, mo.RijMat, dict(prm, csv_dir=str(tmp_path)))
    DESC_init(mo.Ind, mo.RijMat, dict(prm, csv_dir=str(tmp_path)))
    for name in ("linear_convergence_rotation_error.csv", "linear_convergence_svec_error.csv"):
        rows = (tmp_path / name).read_text().strip().split("\n")
        assert len(rows) == 2 and len(rows[0].split(",")) == 5


def test_full_size_c2():
    """C2 (n = 1000, ~2.5e5 variables, ~3.1e7 rows), default tol: the certificates recomputed in NumPy with vectorised gathers over the
    index arrays (no matrix is formed).  The accuracy figures next to DESC()'s are printed, not asserted."""
    mo = Uniform_Topology(1000, 0.5, 0.3, 0.1, "uniform", seed=1)
    Rest, S, info = linprog_sij(mo.Ind, mo.RijMat, dict(seed=SEED, return_dual=True), return_info=True)
    lp = info["lp"]
    tol = 1e-4
    assert lp["converged"] == 1, lp
    pos, k, y = info["pos_edges"], info["k"].astype(np.int64) - 1, info["y"]
    mp, ns = k.shape
    Ind = np.asarray(mo.Ind, dtype=np.int64) - 1
    n = int(Ind.max()) + 1
    key = Ind[:, 0] * n + Ind[:, 1]                                   # sorted: Ind is sorted by (i, j)
    def edge_of(u, v):
        return np.searchsorted(key, np.minimum(u, v) * n + np.maximum(u, v))
    i, j = Ind[pos, 0][:, None], Ind[pos, 1][:, None]
    ea, eb = edge_of(i, k), edge_of(j, k)
    assert np.array_equal(key[ea], np.minimum(i, k) * n + np.maximum(i, k))
    R = np.ascontiguousarray(np.transpose(mo.RijMat, (2, 0, 1)))
    d = np.empty((mp, ns))
    from oracle.desc_pgd_literal import matlab_abs_acos
    for t in range(ns):                                                # S0Mat column by column (linprog_sij.m:88-101)
        Rjk = np.where((j[:, 0] < k[:, t])[:, None, None], R[eb[:, t]], np.transpose(R[eb[:, t]], (0, 2, 1)))
        Rki = np.where((k[:, t] < i[:, 0])[:, None, None], R[ea[:, t]], np.transpose(R[ea[:, t]], (0, 2, 1)))
        Rc = R[pos] @ Rjk @ Rki
        d[:, t] = matlab_abs_acos((Rc[:, 0, 0] + Rc[:, 1, 1] + Rc[:, 2, 2] - 1) / 2) / np.pi
    x_l, sab = S[pos][:, None], S[ea] + S[eb]
    viol = max(float(np.maximum((x_l - sab) - d, (-x_l - sab) + d).max()), 0.0)
    P = float(S[pos].sum())
    var = np.full(Ind.shape[0], -1, dtype=np.int64); var[pos] = np.arange(mp)
    z = y[..., 0] + y[..., 1]
    KTy = (y[..., 0] - y[..., 1]).sum(axis=1) - np.bincount(var[ea].reshape(-1), z.reshape(-1), mp) - np.bincount(var[eb].reshape(-1), z.reshape(-1), mp)
    D = float(-(d * (y[..., 0] - y[..., 1])).sum() + np.minimum(1.0 + KTy, 0.0).sum())
    print("C2: m_pos %d nsample %d rows %d  iters %d restarts %d  viol %.3e  P %.10g  D %.10g  loop %.0f ms (samples %.0f, transpose %.0f)"
          % (mp, ns, lp["rows"], lp["iters"], lp["restarts"], viol, P, D, lp["ms_loop"], lp["ms_samples"], lp["ms_transpose"]))
    assert np.all(y >= 0) and np.all(S >= 0) and np.all(S <= 1)
    assert viol <= tol
    assert P - D <= tol * (1 + abs(P) + abs(D))
    assert abs(lp["pobj"] - P) <= 1e-9 * P and abs(lp["dobj"] - D) <= 1e-9 * abs(D) + 1e-9 * P and abs(lp["viol"] - viol) <= 1e-9
    assert in_so3(info["R_gcw"]) and in_so3(Rest)
    assert info["refine"]["cg_unconverged"] == 0
    R_est, R_init, S_qp = DESC(mo.Ind, mo.RijMat, dict(iters=100, learning_rate=0.01, Gradient=ConstantStepSize(0.01), verbose=False, seed=SEED))
    err = lambda Rr: Rotation_Alignment(Rr, mo.R_orig)[2:]       # noqa: E731
    print("C2 accuracy: mean|S - ErrVec|  LP %.4f  DESC %.4f;  mean/median rotation error (deg)  LP R_gcw %.3f/%.3f  LP Rest %.3f/%.3f  "
          "DESC R_init %.3f/%.3f  DESC R_est %.3f/%.3f" % ((np.abs(S - mo.ErrVec).mean(), np.abs(S_qp - mo.ErrVec).mean()) + err(info["R_gcw"]) + err(Rest)
                                                          + err(R_init) + err(R_est)))

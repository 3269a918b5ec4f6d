"""The Spectral / GCW eigen-solve without a GPU: (1) the NumPy restatements of tests/spectral_kernels_oracle.py are qualified against
the dense oracle (oracle/spectral_oracle.py) and against plain NumPy, (2) the cases of tests/spectral_cases.py are shown to reach the
branches they are named after, (3) the desc_test_spectral_* hooks refuse bad arguments before any device work, and (4) the small dense
helpers of small_dense.h (jacobi_eig, ortho_coeffs, project_so3, ritz_scale_sign + project_nodes) run through the desc_test_small_*
hooks of the mock-runtime build in a child process and are compared with NumPy / LAPACK.

Tolerances of (4) are set against the reference, not the code: for every case the same defect is evaluated for NumPy's own result and
8 times the largest value seen in the case's group is allowed, with a floor of 16 N eps |A| (eps = 2^-52).  Measured when this file was
written (largest value over all cases; "numpy" is what the tolerance is built from):

    jacobi_eig   eigen-residual / |A|_2   ours 1.2e-15   numpy 8.9e-16        V'V - I      ours 2.7e-15   numpy 2.2e-15
    ortho_coeffs C'GC - I                 ours 1.3e-04   numpy 1.1e-04   (column scaling 1e6, cond(G) 1e12; 1.7e-15 / 6.7e-16 at cond ~ 1)
    project_so3  max(|RR' - I|, |det R - 1|) over every finite case, rank-deficient ones included     ours 8.9e-16   numpy 4.0e-15
                 |R - R_numpy| where the projection is unique, in units of NumPy's own sensitivity    at most 7.9 (allowed: 8)
                 -- that distance is NumPy's own error: against the projection from a 50-digit SVD ours is within 3.4e-16, NumPy's
                 within 8.0e-15 on the same blocks, so the 50-digit projection is asserted as well (8 eps cond).

project_so3 before it became a one-sided Jacobi SVD (U = M v / sqrt(eig(M'M))) against the same checks: the orthogonality defect was
1e-12 at sigma_3 / sigma_1 = 1e-2, 9e-9 at 1e-4, 1e-4 at 1e-6, and of order 1 from 1e-8 down and for every exactly rank-deficient block."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.spectral_oracle import _blk, _project
from tests import spectral_cases as K
from tests import spectral_kernels_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------------------------------------------------------- the restatements
def _ind(ii, jj):
    return np.stack([ii, jj], axis=1).astype(np.int64) + 1


def _rijmat(rij):
    return np.transpose(rij.reshape(-1, 3, 3), (2, 1, 0)).copy()              # [r, c, e] = rij[e, r + 3c]


@pytest.mark.parametrize("name", ["er60", "stars64"])
def test_assembled_blocks_are_the_oracles_dense_matrix(name):
    n, ii, jj, rij = K.graphs()[name]
    A = O.dense_from_blocks(n, ii, jj, O.assemble(n, ii, jj, rij))
    assert np.array_equal(A, _blk(_ind(ii, jj), _rijmat(rij), n))
    assert np.array_equal(A, A.T)


def test_assembled_gcw_blocks_are_the_symmetric_form_of_the_oracles_matrix():
    """GCW.m:20-23 builds D^-1 (W o B); the library iterates D^-1/2 (W o B) D^-1/2.  Entry by entry the restatement is the oracle's
    matrix up to the three roundings of its scale factor, and the two have the same spectrum."""
    n, ii, jj, rij = K.er_graph()
    S = np.random.default_rng(1).uniform(2e-3, 1.0, size=len(ii))
    w = O.gcw_weights(S)
    assert np.allclose(w, 1.0 / (S ** 1.5 + 1e-8), rtol=4 * EPS, atol=0)
    deg, _ = O.row_wsum(n, ii, jj, w)
    dinv = 1.0 / np.sqrt(deg)
    A = O.dense_from_blocks(n, ii, jj, O.assemble(n, ii, jj, rij, w, dinv))
    Wm = np.zeros((n, n)); Wm[ii, jj] = w; Wm = Wm + Wm.T
    assert np.allclose(deg, Wm.sum(axis=1), rtol=64 * EPS, atol=0)
    B = _blk(_ind(ii, jj), _rijmat(rij), n) * np.kron(Wm, np.ones((3, 3)))
    D = np.kron(np.diag(dinv), np.eye(3))
    assert np.allclose(A, D @ B @ D, rtol=8 * EPS, atol=0) and np.array_equal(A, A.T)
    row_normalised = np.kron(np.diag(1.0 / Wm.sum(axis=1)), np.eye(3)) @ B                 # the oracle's RijW
    lam = np.sort(np.linalg.eigvals(row_normalised).real)[::-1]
    assert np.abs(lam[:6] - np.linalg.eigvalsh(A)[::-1][:6]).max() < 1e-12


@pytest.mark.parametrize("pname", list(K.spmm_params()))
def test_spmm_restatement_is_the_dense_product(pname):
    n, ii, jj, rij = K.er_graph()
    alpha, s1, s2, zk, _ = K.spmm_params()[pname]
    blocks = O.assemble(n, ii, jj, rij, K.edge_weights(len(ii), "wide"))
    x = K.operand(n, 1)
    z = x if zk == "x" else K.operand(n, 2) if zk == "other" else np.full_like(x, np.nan)
    y, bound = O.spmm(n, ii, jj, blocks, x, z, alpha, s1, s2)
    A = O.dense_from_blocks(n, ii, jj, blocks)
    plain = alpha * (A @ x) + s1 * x + (s2 * z if s2 != 0.0 else 0.0)
    assert np.isfinite(y).all() and (np.abs(plain - y) <= 4 * bound + 1e-300).all()        # BLAS may fuse: a loose qualification
    assert (bound > 0).all()
    # with weights of one size a lost slot is ten orders of magnitude outside the bound
    blocks = O.assemble(n, ii, jj, rij)
    y, bound = O.spmm(n, ii, jj, blocks, x, z, alpha, s1, s2)
    rp, adj, _ = O.csr(n, ii, jj)
    v = int(np.argmax(rp[1:] - rp[:-1])); t = rp[v]
    lost = alpha * (blocks[:, t].reshape(3, 3).T @ x[3 * adj[t]:3 * adj[t] + 3])
    assert (np.abs(lost) / bound[3 * v:3 * v + 3]).max() > 1e10


def test_sum_restatements_against_numpy():
    rng = np.random.default_rng(2)
    X, Y = rng.standard_normal((257, 6)), rng.standard_normal((257, 6))
    G1, G2, b1, b2 = O.gram(X, Y)
    assert (np.abs(G1 - X.T @ Y) <= b1).all() and (np.abs(G2 - Y.T @ Y) <= b2).all()
    Z3, theta = rng.standard_normal((6, 3)), rng.standard_normal(3)
    nrm, bound = O.residual(X, Y, Z3, theta)
    assert (np.abs(nrm - np.linalg.norm(Y @ Z3 - (X @ Z3) * theta, axis=0)) <= bound).all()
    Cm = rng.standard_normal((6, 6))
    assert np.allclose(O.combine(Y, Cm), Y @ Cm, rtol=0, atol=16 * EPS * (np.abs(Y) @ np.abs(Cm)).max())
    n, ii, jj, _ = K.er_graph()
    w = K.edge_weights(len(ii), "wide")
    deg, bound = O.row_wsum(n, ii, jj, w)
    Wm = np.zeros((n, n)); Wm[ii, jj] = w; Wm = Wm + Wm.T
    assert (np.abs(deg - Wm.sum(axis=1)) <= bound).all()
    assert np.array_equal(O.row_wsum(n, ii, jj)[0], O.slots(n, ii, jj).astype(np.float64))


def test_weight_restatement_at_the_special_values():
    w = O.gcw_weights(K.S_VALUES)
    assert w[0] == 1.0 / 1e-8 and w[1] == 1.0 / 1e-8 and w[5] == 0.0 and np.isnan(w[6]) and np.isnan(w[7])
    assert np.allclose(w[2:5], 1.0 / (np.array(K.S_VALUES[2:5]) ** 1.5 + 1e-8), rtol=4 * EPS, atol=0)


def test_the_near_eigenpair_case_needs_the_explicit_residual():
    X, Y, Z3, theta = K.residual_near_eigenpair(257)
    nrm, bound = O.residual(X, Y, Z3, theta)
    assert (nrm > 1e-12).all() and (nrm < 1e-10).all() and (bound <= 1e-2 * nrm).all()       # two digits are within reach
    gram_form = np.sqrt(np.abs(np.einsum("rc,rc->c", Y @ Z3, Y @ Z3) - theta ** 2))
    assert (np.abs(gram_form - nrm) > 10 * nrm).any()


# ---------------------------------------------------------------------------------------------------------------- the cases
def test_star_forests_sit_on_the_slot_edges():
    for leaves, tpr in ((K.LEAVES_64, 64), (K.LEAVES_256, 256)):
        n, ii, jj, rij, centres = K.star_forest(leaves)
        assert n < 2500
        sl = O.slots(n, ii, jj)
        assert [int(sl[c]) for c in centres] == list(leaves)
        have = set(leaves)
        assert {tpr - 1, tpr, tpr + 1, 2 * tpr - 1, 2 * tpr, 2 * tpr + 1} <= have
        rp, adj, _ = O.csr(n, ii, jj)
        for c, L in zip(centres, leaves):
            if L >= 2:
                nb = adj[rp[c]:rp[c + 1]]
                assert (nb < c).any() and (nb > c).any()               # both branches of assembly in one row
        assert 2 * len(ii) < 192 * n                                   # the product path's rule picks the wave-per-row kernel here
    n, ii, jj, _, centres = K.star_forest(K.LEAVES_64)
    assert O.slots(n, ii, jj)[centres[0]] == 0                         # the isolated node
    for g in (1, 3):                                                   # forced grids make every stride loop turn at these sizes
        assert g * 4 < n and g * 16 < n


def test_inputs_span_what_they_are_named_after():
    n, ii, jj, _ = K.er_graph()
    w = K.edge_weights(len(ii), "wide")
    assert w.max() / w.min() > 1e14 and w.min() > 0
    d = K.dinv_with_zeros(n)
    assert (d == 0).sum() >= 3 and (d > 0).sum() >= 3
    P = K.spmm_params()
    assert all(v != 0 for v in P["cheb2"][:3]) and P["cheb1"][2] == 0 and P["nan_z"][2] == 0 and P["z_is_y"][4]
    assert 65536 in K.ROW_COUNTS and any(r % 3 for r in K.ROW_COUNTS)


def test_project_cases_have_the_ranks_and_conditions_they_claim():
    C = K.project_cases()
    sv = lambda M: np.linalg.svd(M, compute_uv=False)
    for s3 in K.SIGMA3:
        for tag, sg in (("+", 1.0), ("-", -1.0)):
            for M in C[f"ladder{tag}{s3:g}"]:
                s = sv(M)
                assert np.abs(s - np.sort([1.0, 0.7, s3])[::-1]).max() < 1e-14
                if s3 >= 1e-13:
                    assert np.sign(np.linalg.det(M)) == sg
                exp = np.sort([1.0, 0.7, s3])[::-1]
                assert O.projection_is_unique(M) == (exp[1] + sg * exp[2] >= 1e-6)
    assert all(np.linalg.matrix_rank(M) == 2 for M in C["rank2_exact"]) and all(sv(M)[2] == 0 for M in C["rank2_exact"])
    assert all(sv(M)[2] < 1e-15 * sv(M)[0] for M in C["rank2"])
    assert all(np.linalg.matrix_rank(M) == 1 for M in C["rank1_exact"]) and all(np.linalg.matrix_rank(M) == 1 for M in C["rank1_axis"])
    assert not C["zero"].any()
    assert np.abs(C["scale1e-100"]).max() < 1e-99 and np.abs(C["scale1e100"]).min() > 1e96
    assert max(O.so3_defect(M) for M in C["rotation"]) < 1e-14


def test_exit_inputs_have_a_gap_below_the_third_eigenvalue():
    """tests/test_gpu_spectral_exits.py bounds |theta_c - lambda_c| by the residual: that needs lambda_3 - lambda_4 > 1e-3 scale."""
    for name in K.exit_inputs():
        A, sigma = K.exit_dense(name)
        assert np.array_equal(A, A.T)
        lam = np.linalg.eigvalsh(A)[::-1]
        assert lam[2] - lam[3] > 1e-3 * max(abs(lam[0]), sigma), (name, lam[:5])
    assert K.exit_problem()[1] <= 150


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_hooks_refuse_bad_arguments_before_any_device_work(lib):
    L = lib.load()
    d = np.zeros(64); p = lib.ptr(d, lib.F64P)
    i32 = np.zeros(8, dtype=np.int32); pi = lib.ptr(i32, lib.I32P)
    calls = [
        L.desc_test_spectral_weights(None, 1, 0, p), L.desc_test_spectral_weights(p, 1, 0, None), L.desc_test_spectral_weights(p, -1, 0, p),
        L.desc_test_spectral_row_wsum(None, p, 1, 0, p), L.desc_test_spectral_assemble(None, p, p, 1, 0, p),
        L.desc_test_spectral_spmm(None, p, p, p, 0, 0, 0, 1.0, 0.0, 0.0, p),
        L.desc_test_spectral_gram(None, p, 1, 0, 0, p, p), L.desc_test_spectral_gram(p, p, 1, 0, 0, None, p), L.desc_test_spectral_gram(p, p, -1, 0, 0, p, p),
        L.desc_test_spectral_gram(p, p, 1, -1, 0, p, p), L.desc_test_spectral_gram(p, p, 1, 65536, 0, p, p),
        L.desc_test_spectral_residual(p, None, 1, p, p, 0, 0, p), L.desc_test_spectral_residual(p, p, 1, None, p, 0, 0, p),
        L.desc_test_spectral_residual(p, p, -1, p, p, 0, 0, p), L.desc_test_spectral_residual(p, p, 1, p, p, 65536, 0, p),
        L.desc_test_spectral_combine(None, 1, p, 0, 0, p), L.desc_test_spectral_combine(p, -1, p, 0, 0, p), L.desc_test_spectral_combine(p, 1, p, -2, 0, p),
        L.desc_test_small_jacobi(4, p, p, p), L.desc_test_small_jacobi(3, None, p, p), L.desc_test_small_ortho(None, p, p, pi),
        L.desc_test_small_ortho(p, p, p, None), L.desc_test_small_project(None, 1, p), L.desc_test_small_project(p, -1, p),
        L.desc_test_small_ritz_tail(None, p, 1, p), L.desc_test_small_ritz_tail(p, p, 0, p),
    ]
    assert all(rc == lib.ERR_INVALID for rc in calls), calls
    assert L.desc_last_error()


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from desc_amd import _lib as lib
from tests import spectral_cases as K
L = lib.load()
assert hasattr(L, "hipmock_launch_count"), "must run against the mock build"
out = {}
# ---- argument checks on a device problem of the mock runtime: nothing may be launched
n, ii, jj, rij = K.tiny_graph(5)
dp = lib.DeviceProblem(lib.ProblemArrays(n, ii, jj, rij.reshape(-1)))
m, h = dp.m, dp.handle
d = np.zeros(18 * 64); p = lib.ptr(d, lib.F64P)
c0 = L.hipmock_launch_count()
out["refused"] = [
    L.desc_test_spectral_row_wsum(h, p, m + 1, 0, p), L.desc_test_spectral_row_wsum(h, p, m, -1, p), L.desc_test_spectral_row_wsum(h, p, m, 65536, p),
    L.desc_test_spectral_row_wsum(h, p, m, 0, None),
    L.desc_test_spectral_assemble(h, p, p, m - 1, 0, p), L.desc_test_spectral_assemble(h, p, p, m, 70000, p), L.desc_test_spectral_assemble(h, p, p, m, 0, None),
    L.desc_test_spectral_spmm(h, None, p, p, 0, 0, 0, 1.0, 0.0, 0.0, p), L.desc_test_spectral_spmm(h, p, None, p, 0, 0, 0, 1.0, 0.0, 0.0, p),
    L.desc_test_spectral_spmm(h, p, p, None, 0, 0, 0, 1.0, 0.0, 0.0, p), L.desc_test_spectral_spmm(h, p, p, p, 0, 0, 0, 1.0, 0.0, 0.0, None),
    L.desc_test_spectral_spmm(h, p, p, p, 0, 1, 0, 1.0, 0.0, 0.0, p), L.desc_test_spectral_spmm(h, p, p, p, 0, 128, 0, 1.0, 0.0, 0.0, p),
    L.desc_test_spectral_spmm(h, p, p, p, 0, 64, -1, 1.0, 0.0, 0.0, p),
]
out["refused_launches"] = L.hipmock_launch_count() - c0
out["invalid"] = lib.ERR_INVALID
# the wrappers end to end (no kernel runs: device blocks read back as zeros): sizes and guard words
c0 = L.hipmock_launch_count()
assert lib.hook_spectral_weights(np.ones(7)).shape == (7,)
assert lib.hook_spectral_row_wsum(dp, None, grid=1).shape == (n,) and lib.hook_spectral_row_wsum(dp, np.ones(m)).shape == (n,)
blocks = lib.hook_spectral_assemble(dp, np.ones(m), np.ones(n), grid=3)
assert blocks.shape == (9, 2 * m)
x = K.operand(n, 1)
for form in (0, 64, 256):
    assert lib.hook_spectral_spmm(dp, blocks, x, x, 1.0, 0.5, 0.25, z_is_y=(form == 64), form=form, grid=form // 64).shape == (3 * n, 6)
G1, G2 = lib.hook_spectral_gram(x, x, grid=2)
assert G1.shape == (6, 6) and G2.shape == (6, 6)
assert lib.hook_spectral_residual(x, x, np.eye(6)[:, :3], np.ones(3)).shape == (3,)
assert lib.hook_spectral_combine(x, np.eye(6), grid=1).shape == (3 * n, 6)
out["ok_launches"] = L.hipmock_launch_count() - c0
# ---- the small dense helpers: host code, the same text the GPU build runs
c0 = L.hipmock_launch_count()
out["jacobi"] = {k: [[a.tolist() for a in lib.hook_small_jacobi(A)] for A in v] for k, v in K.jacobi_cases().items()}
good = {}
for k, (G, Z) in K.ortho_good_cases().items():
    ok, Cm = lib.hook_small_ortho(G, Z)
    good[k] = [ok, Cm.tolist()]
out["ortho_good"] = good
out["ortho_bad"] = {k: lib.hook_small_ortho(G)[0] for k, G in K.ortho_bad_cases().items()}
out["project"] = {k: lib.hook_small_project(M).tolist() for k, M in K.project_cases().items()}
tails = {}
for k, (V, dinv) in K.ritz_tail_cases().items():
    tails[k] = lib.hook_small_ritz_tail(V, dinv).tolist()
out["tail"] = tails
# one node: answered before any device work
e32 = np.zeros(0, dtype=np.int32)
R1, i1 = lib.spectral_run(lib.ProblemArrays(1, e32, e32, np.zeros(0)), None, True)
out["n1"] = [R1[:, :, 0].tolist(), i1["converged"], i1["iters"], i1["products"], i1["residual"], i1["eigenvalues"]]
out["small_launches"] = L.hipmock_launch_count() - c0
print("RESULT " + json.dumps(out))
"""


@functools.lru_cache(maxsize=None)
def _child():
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipmock"))
    import build_host
    so = build_host.build(ROOT, "none")
    env = dict(os.environ, DESC_AMD_LIB=so, OPENBLAS_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])


def test_dp_hooks_refuse_bad_arguments_on_the_mock_runtime():
    """A wrong m, a grid outside [0, 65535], an unknown form and a NULL array are refused before anything is launched; good calls
    launch, and the Python wrappers run end to end."""
    out = _child()
    assert out["refused"] and all(rc == out["invalid"] for rc in out["refused"]), out["refused"]
    assert out["refused_launches"] == 0 and out["ok_launches"] >= 9 and out["small_launches"] == 0


def test_one_node_is_answered_without_the_device():
    """n = 1: the 3 x 6 start block cannot have full rank; the answer is the identity, converged, with no iteration and no product."""
    assert _child()["n1"] == [np.eye(3).tolist(), True, 0, 0, 0.0, [0.0, 0.0, 0.0]]


# ---------------------------------------------------------------------------------------------------------------- small dense helpers
@pytest.mark.parametrize("group", list(K.jacobi_cases()))
def test_jacobi_eig_against_eigh(group):
    mats = K.jacobi_cases()[group]
    got = _child()["jacobi"][group]
    N = mats[0].shape[0]
    ref_res = ref_orth = 0.0
    for A in mats:
        As = 0.5 * (A + A.T)
        lam, vec = np.linalg.eigh(As)
        r, o = O.eig_defects(As, lam, vec)
        nrm = np.linalg.norm(As, 2)
        ref_res = max(ref_res, r / max(nrm, 1e-300)); ref_orth = max(ref_orth, o)
    for A, (w, V) in zip(mats, got):
        w, V = np.array(w), np.array(V)
        As = 0.5 * (A + A.T)                                           # an asymmetric input is symmetrised
        nrm = np.linalg.norm(As, 2)
        assert (np.diff(w) <= 0).all()                                 # descending
        r, o = O.eig_defects(As, w, V)
        assert r <= max(8 * ref_res, 16 * N * EPS) * nrm, (group, r, ref_res * nrm)
        assert o <= max(8 * ref_orth, 16 * N * EPS), (group, o, ref_orth)
        lam = np.linalg.eigvalsh(As)[::-1]
        assert np.abs(w - lam).max() <= max(8 * ref_res, 16 * N * EPS) * nrm
    if group.startswith(("diagonal", "equal", "zero")):
        for A, (w, V) in zip(mats, got):                               # nothing to rotate: V is a permutation, equal values keep their index order
            order = sorted(range(N), key=lambda i: -A[i, i])           # stable
            assert np.array_equal(np.array(w), np.diag(A)[order]) and np.array_equal(np.array(V), np.eye(N)[:, order])


def test_ortho_coeffs_against_cholesky():
    got = _child()
    ref = {k: O.ortho_defect(G, O.ortho_numpy(G, Z)) for k, (G, Z) in K.ortho_good_cases().items()}
    for k, (G, Z) in K.ortho_good_cases().items():
        ok, Cm = got["ortho_good"][k]
        assert ok, k
        Cm = np.array(Cm)
        group = k.split("_")[0]
        allowed = max(8 * max(v for kk, v in ref.items() if kk.split("_")[0] == group), 16 * 6 * EPS)
        dft = O.ortho_defect(G, Cm)
        assert dft <= allowed, (k, dft, allowed)
        Zm = np.eye(6) if Z is None else Z
        T = np.linalg.solve(Zm, Cm)                                    # C = Z L^-T: Z^-1 C is upper triangular with a positive diagonal
        assert np.abs(np.tril(T, -1)).max() <= 64 * EPS * np.abs(T).max() and (np.diag(T) > 0).all()
    assert np.linalg.cond(K.ortho_good_cases()["scale1e+06_I"][0]) > 1e11
    assert got["ortho_bad"] == {k: False for k in K.ortho_bad_cases()}


@pytest.mark.parametrize("group", list(K.project_cases()))
def test_project_so3_against_the_svd_projection(group):
    Ms = K.project_cases()[group]
    Rs = np.array(_child()["project"][group])
    for M, R in zip(Ms, Rs):
        ref = O.so3_defect(O.project_numpy(M))
        dft = O.so3_defect(R)
        assert dft <= max(8 * ref, 16 * EPS), (group, dft, ref)
        if O.projection_is_unique(M):
            sens = O.projection_sensitivity(M)
            diff = float(np.abs(R - O.project_numpy(M)).max())
            assert diff <= 8 * max(sens, EPS), (group, diff, sens)
            # and against the projection from a 50-digit SVD: a backward-stable result moves by the condition of the projection,
            # sigma_1 / (sigma_2 + sign(det M) sigma_3), times a few eps
            s = np.linalg.svd(M, compute_uv=False)
            cond = s[0] / (s[1] + np.sign(np.linalg.det(M / s[0])) * s[2])
            assert np.abs(R - O.project_exact(M)).max() <= 8 * EPS * cond, (group, cond)
    if group == "zero":
        assert np.array_equal(Rs[0], np.eye(3))
    if group == "rotation":
        assert np.abs(Rs - Ms).max() <= 16 * EPS


@pytest.mark.parametrize("name", list(K.ritz_tail_cases()))
def test_ritz_tail_is_the_oracles_projection(name):
    """ritz_scale_sign + project_nodes against oracle/spectral_oracle.py::_project on the vectors scaled and normalised in NumPy."""
    V, dinv = K.ritz_tail_cases()[name]
    n = V.shape[0] // 3
    R = np.array(_child()["tail"][name])
    W = V * (np.repeat(dinv, 3)[:, None] if dinv is not None else 1.0)
    W = W / np.linalg.norm(W, axis=0)
    assert (np.linalg.det(W[:3]) < 0) == name.endswith("neg")
    Rref = _project(W, n)
    for v in range(n):
        blk = W[3 * v:3 * v + 3] * np.array([np.sign(np.linalg.det(W[:3])), 1.0, 1.0])
        assert O.projection_is_unique(blk)
        assert np.abs(R[:, :, v] - Rref[:, :, v]).max() <= 8 * max(O.projection_sensitivity(blk), EPS) + 8 * EPS
        assert O.so3_defect(R[:, :, v]) <= max(8 * O.so3_defect(Rref[:, :, v]), 16 * EPS)

"""GPU tests of the batched CEMP baselines (desc_cemp_batch_*, desc_mst_batch_run; CEMP_batch, CEMP_GCW_batch, MST_batch,
CEMP_MST_batch): every problem of a batch bit for bit against the single call and at 1e-12 against the NumPy restatement (the tolerance
of tests/test_gpu_cemp.py), the bitwise independence of a problem's result from the batch around it, the three nsample classes of the
round, per-problem seeds, handle reuse, the eigen-solve composition (1e-8 after alignment, as tests/test_gpu_gcw_batch.py) and the tree
step against Kruskal and MST()."""
import numpy as np
import pytest
import scipy.linalg

from desc_amd import CEMP, CEMP_GCW, MST, Rotation_Alignment
from desc_amd.algorithms import marshal_edges
from oracle.spectral_oracle import _blk, _project, rotation_alignment
from tests import cemp_batch_cases as cases
from tests.mpls_oracle import kruskal

pytestmark = pytest.mark.gpu

MAIN = [k for k in cases.NAMES if k != "hub300"]          # the eleven; U40 goes in with its rows permuted, Ind as Fortran-ordered doubles
WIDE = ["hub300", "U100d"]                                # a row above 64 and above 256 entries, codegrees above 64
SMALL = ["U12", "band10_2", "pend30"]


def problem(name):
    if name == "U40":
        return cases.permuted("U40")[:2]
    mo = cases.model(name)
    return mo.Ind, mo.RijMat


def sorted_order(name, v):
    """A per-edge vector in the caller's order -> the order of the model's Ind."""
    if name != "U40":
        return v
    out = np.empty_like(v); out[cases.permuted("U40")[2]] = v
    return out


def assert_rotations(R):
    Rm = np.transpose(R, (2, 0, 1))
    assert np.isfinite(Rm).all()
    assert np.abs(Rm @ np.transpose(Rm, (0, 2, 1)) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(Rm) - 1).max() < 1e-12


def aligned_diff(R, R_ref):
    return float(np.abs(rotation_alignment(R, R_ref)[0] - R_ref).max())


@pytest.fixture(scope="module")
def solved():
    """The two batches, solved once through the public entry point: name -> SVec in the caller's order."""
    from desc_amd import CEMP_batch
    out = {}
    for names in (MAIN, WIDE):
        out.update(zip(names, CEMP_batch([problem(k) for k in names], cases.params())))
    return out


# ---- 1. parity with the single call and the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("names", [MAIN, WIDE], ids=["eleven", "wide_rows"])
def test_batch_equals_single_call_and_oracle(solved, names):
    for k in names:
        S = solved[k]
        single = CEMP(*problem(k), cases.params())
        ref = cases.oracle_S(k)
        err = float(np.abs(sorted_order(k, S) - ref).max())
        print(k, S.shape[0], "equal to CEMP():", np.array_equal(S, single), "max |S - oracle|:", err)
        assert np.array_equal(S, single), k
        assert err < 1e-12, (k, err)
        assert np.array_equal(sorted_order(k, S) == 1.0, cases.no_cycle(k)), k      # exactly the edges without a 3-cycle
    if names == MAIN:
        assert cases.no_cycle("bridged").sum() == 2 and np.array_equal(cases.no_cycle("bridged"), cases.model("bridged").bridge)
        assert cases.no_cycle("pend30").sum() == 4 and cases.no_cycle("star12").all() and cases.no_cycle("U278").sum() == 345
        assert not any(cases.no_cycle(k).any() for k in ("U8", "U12", "U40", "U90", "U150"))


# ---- 2. independence from the batch --------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_batch_around_it(solved):
    """As given, reversed, and each problem alone (another grid and another LDS size per launch): the same bits."""
    from desc_amd import CEMP_batch
    rev = CEMP_batch([problem(k) for k in reversed(MAIN)], cases.params())
    for k, S in zip(reversed(MAIN), rev):
        assert np.array_equal(S, solved[k]), k
    for k in MAIN + WIDE:
        assert np.array_equal(CEMP_batch([problem(k)], cases.params())[0], solved[k]), k


# ---- 3. the nsample classes of the round ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsample", [1, 64, 65, 256, 257])
def test_nsample_classes(nsample):
    from desc_amd import CEMP_batch
    par = cases.params(nsample=nsample)
    got = CEMP_batch([problem(k) for k in SMALL], par)
    for k, S in zip(SMALL, got):
        err = float(np.abs(S - cases.oracle_S(k, nsample=nsample, literal=True)).max())
        print(nsample, k, err)
        assert err < 1e-12, (k, err)
        assert np.array_equal(S, CEMP(*problem(k), par)), k


# ---- 4. per-problem seeds and parameter edges ----------------------------------------------------------------------------------
def test_per_problem_seeds_and_parameter_edges(solved):
    from desc_amd import CEMP_batch
    probs = [problem(k) for k in SMALL]
    got = CEMP_batch(probs, cases.params(), seeds=[3, 4, 5])
    for k, S, seed in zip(SMALL, got, (3, 4, 5)):
        assert np.array_equal(S, CEMP(*problem(k), cases.params(seed=seed))), k
        assert np.abs(S - cases.oracle_S(k, seed=seed)).max() < 1e-12, k
    assert not np.array_equal(got[0], solved["U12"]) and not np.array_equal(got[2], solved["pend30"])      # seed 1 gives other samples
    par = cases.params(max_iter=5, reweighting=[1.0, 4.0])                  # missing betas repeat the last one (CEMP.m:30-34)
    for k, S in zip(SMALL, CEMP_batch(probs, par)):
        assert np.array_equal(S, CEMP(*problem(k), par)), k
        assert np.abs(S - cases.oracle_S(k, max_iter=5, reweighting=[1.0, 4.0])).max() < 1e-12, k
    par0 = cases.params(max_iter=0)                                         # the initial means (:102-103)
    for k, S in zip(SMALL, CEMP_batch(probs, par0)):
        assert np.array_equal(S, CEMP(*problem(k), par0)), k
        assert np.abs(S - cases.oracle_S(k, max_iter=0)).max() < 1e-12, k
    with_info = CEMP_batch(probs, cases.params(), return_info=True)
    assert all(np.array_equal(S, solved[k]) and info["timings"]["ms_build"] > 0 for k, (S, info) in zip(SMALL, with_info))


# ---- 5. more problems than compute units --------------------------------------------------------------------------------------
def test_more_problems_than_compute_units():
    from desc_amd import CEMP_batch
    from oracle.cemp_oracle import cemp_oracle_batched
    mos = cases.many_small(300)
    got = CEMP_batch(mos, cases.params())
    worst = max(float(np.abs(S - cemp_oracle_batched(mo.Ind, mo.RijMat, 6, cases.BETA, 50, 1)).max()) for mo, S in zip(mos, got))
    print("worst |S - oracle| over 300 problems:", worst)
    assert worst < 1e-12


# ---- 6. handle reuse and the sampled structure -------------------------------------------------------------------------------
def test_handle_reuse_and_samples(lib, solved):
    names = ["U12", "pend30", "U90"]
    probs = []
    for k in names:
        n, ii, jj, rij, perm = marshal_edges(*problem(k))
        assert perm is None
        probs.append(lib.ProblemArrays(n, ii, jj, rij))
    h = lib.CempBatch(probs, 50, seed=1)
    first = [S.copy() for S in h.run(cases.BETA, 6)[0]]
    second = [S.copy() for S in h.run([1.0, 4.0], 5)[0]]
    again = [S.copy() for S in h.run(cases.BETA, 6)[0]]
    smp = h.samples()
    means = [S.copy() for S in h.run(cases.BETA, 0)[0]]
    h.destroy()
    for beta, it, got in ((cases.BETA, 6, first), ([1.0, 4.0], 5, second), (cases.BETA, 6, again)):
        f = lib.CempBatch(probs, 50, seed=1)
        fresh = f.run(beta, it)[0]
        assert all(np.array_equal(a, b) for a, b in zip(got, fresh))
        f.destroy()
    assert all(np.array_equal(a, solved[k]) for a, k in zip(first, names))
    assert not np.array_equal(first[0], second[0])
    # what create sampled: local edge ids of the two other edges of a triangle through the same third node; S0's column means
    for k, q, s, mean in zip(names, probs, smp, means):
        hc = s["has_cycle"]
        assert np.array_equal(~hc, cases.no_cycle(k)), k
        assert (s["e_jk"][~hc] == -1).all() and (s["e_ki"][~hc] == -1).all() and (s["s0"][~hc] == 0).all()
        ejk, eki = s["e_jk"][hc], s["e_ki"][hc]
        assert ejk.min() >= 0 and ejk.max() < q.m and eki.min() >= 0 and eki.max() < q.m
        i, j = q.ind_i[hc][:, None], q.ind_j[hc][:, None]
        k_from_i = np.where(q.ind_i[eki] == i, q.ind_j[eki], q.ind_i[eki])          # the other end of the edge at i
        k_from_j = np.where(q.ind_i[ejk] == j, q.ind_j[ejk], q.ind_i[ejk])
        assert ((q.ind_i[eki] == i) | (q.ind_j[eki] == i)).all() and ((q.ind_i[ejk] == j) | (q.ind_j[ejk] == j)).all()
        assert np.array_equal(k_from_i, k_from_j), k
        assert np.abs(s["s0"][hc].mean(axis=1) - mean[hc]).max() < 1e-14 and (mean[~hc] == 1.0).all()


# ---- 7. CEMP_GCW_batch ---------------------------------------------------------------------------------------------------------
GCW_NAMES = [k for k in MAIN if k != "bridged"]           # bridged: gap lambda_3 - lambda_4 of 0.002, not a yardstick for the eigen-solve


def test_cemp_gcw_batch(solved):
    from desc_amd import CEMP_GCW_batch
    probs = [problem(k) for k in GCW_NAMES]
    out = CEMP_GCW_batch(probs, cases.params(), return_info=True)
    plain = CEMP_GCW_batch(probs, cases.params())
    for k, (R, S, info), Rp in zip(GCW_NAMES, out, plain):
        assert np.array_equal(S, solved[k]) and np.array_equal(R, Rp), k
        assert info["gcw"]["converged"] and "ms_eig" in info["gcw"]["timings"] and "ms_build" in info["cemp"]["timings"], k
        assert_rotations(R)
        d = aligned_diff(R, CEMP_GCW(*problem(k), cases.params()))
        print(k, R.shape[2], info["gcw"]["iters"], d)
        assert d < 1e-8, (k, d)
    # U40 against the dense solve of CEMP_GCW.m:137-160 (tests/test_gpu_mpls.py::test_cemp_gcw_matches_dense_oracle)
    mo, n = cases.model("U40"), 40
    S = sorted_order("U40", solved["U40"])
    A = np.zeros((n, n)); Sm = np.zeros((n, n))
    A[mo.Ind[:, 0] - 1, mo.Ind[:, 1] - 1] = 1; A = A + A.T
    Sm[mo.Ind[:, 0] - 1, mo.Ind[:, 1] - 1] = S; Sm = Sm + Sm.T
    W = (1.0 / (Sm + 1e-8)) * A
    W = np.diag(1.0 / W.sum(axis=1)) @ W
    lam, vec = scipy.linalg.eig(_blk(mo.Ind, mo.RijMat, n) * np.kron(W, np.ones((3, 3))))
    V = np.real(vec[:, np.argsort(-lam.real)[:3]])
    ref = _project(V / np.linalg.norm(V, axis=0), n)
    d = float(np.abs(Rotation_Alignment(out[GCW_NAMES.index("U40")][0], ref)[0] - ref).max())
    print("U40 against the dense solve:", d)
    assert d < 1e-7
    # independence from the batch
    rev = CEMP_GCW_batch(probs[::-1], cases.params())
    for b, k in enumerate(GCW_NAMES):
        assert np.array_equal(rev[len(probs) - 1 - b], plain[b]), k
        assert np.array_equal(CEMP_GCW_batch([probs[b]], cases.params())[0], plain[b]), k


# ---- 8. MST_batch / CEMP_MST_batch ---------------------------------------------------------------------------------------------
def test_mst_batch(solved):
    from desc_amd import CEMP_MST_batch, MST_batch
    names = MAIN + WIDE                                                     # every one is connected; U278: tied keys, star12: all keys equal
    probs = [problem(k) for k in names]
    S = [solved[k] for k in names]
    out = MST_batch(probs, S, return_info=True)
    plain = MST_batch(probs, S)
    perm40 = cases.permuted("U40")[2]
    for k, (R, info), Rp, s in zip(names, out, plain, S):
        tree = kruskal(cases.model(k).Ind, sorted_order(k, s))
        rows = info["tree_edges"]
        assert np.array_equal(np.sort(perm40[rows]) if k == "U40" else rows, tree), k          # a permuted problem: rows of the caller's Ind
        assert np.array_equal(rows, np.sort(rows)), k
        R1, info1 = MST(*problem(k), s, return_info=True)
        assert np.array_equal(R, R1) and np.array_equal(rows, info1["tree_edges"]) and np.array_equal(R, Rp), k
    # tied keys are there: U278's 345 edges without a cycle all carry fl(1 + 1)
    assert np.unique(sorted_order("U278", solved["U278"]) + 1.0).size <= cases.model("U278").Ind.shape[0] - 344
    # U40 with all-equal, increasing and decreasing weights
    mo = cases.model("U40")
    m = mo.Ind.shape[0]
    W = [np.zeros(m), np.arange(m) / m, 1.0 - np.arange(m) / m]
    for w, (R, info) in zip(W, MST_batch([mo] * 3, W, return_info=True)):
        assert np.array_equal(info["tree_edges"], kruskal(mo.Ind, w))
        assert np.array_equal(R, MST(mo.Ind, mo.RijMat, w))
    # independence from the batch
    rev = MST_batch(probs[::-1], S[::-1], return_info=True)
    for b, k in enumerate(names):
        for other in (rev[len(names) - 1 - b], MST_batch([probs[b]], [S[b]], return_info=True)[0]):
            assert np.array_equal(other[0], out[b][0]) and np.array_equal(other[1]["tree_edges"], out[b][1]["tree_edges"]), k
    # the composition
    for names2 in (MAIN, WIDE):
        full = CEMP_MST_batch([problem(k) for k in names2], cases.params(), return_info=True)
        init = CEMP_MST_batch([problem(k) for k in names2], cases.params())
        for k, (R, s, info), Ri in zip(names2, full, init):
            b = names.index(k)
            assert np.array_equal(s, solved[k]) and np.array_equal(R, out[b][0]) and np.array_equal(Ri, R), k
            assert np.array_equal(info["mst"]["tree_edges"], out[b][1]["tree_edges"]) and "ms_tree" in info["mst"]["timings"], k

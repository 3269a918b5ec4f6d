"""GPU tests of the batched Spectral / GCW eigen-solve (desc_gcw_batch_*, Spectral_batch, GCW_batch, DESC_init_batch): every problem of a
batch against the dense LAPACK restatements, the bitwise independence of a problem's result from the batch around it, degenerate
spectra, an empty CSR row, the iteration cap, handle reuse.  Tolerances as tests/test_gpu_spectral.py: rotations compared after
rotation_alignment, max |R_aligned - R_ref| < 1e-8; |RR' - I| and |det - 1| < 1e-12."""
import numpy as np
import pytest

from desc_amd import ConstantStepSize, Rotation_Alignment
from desc_amd.algorithms import marshal_edges
from oracle.spectral_oracle import gcw_oracle, rotation_alignment, spectral_oracle
from tests import graph_shapes as gs
from tests import gcw_batch_cases as cases

pytestmark = pytest.mark.gpu

INFO_KEYS = ("iters", "products", "residual", "eigenvalues", "converged")


def aligned_diff(R, R_ref):
    return float(np.abs(rotation_alignment(R, R_ref)[0] - R_ref).max())


def assert_rotations(R):
    Rm = np.transpose(R, (2, 0, 1))
    assert np.isfinite(Rm).all()
    assert np.abs(Rm @ np.transpose(Rm, (0, 2, 1)) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(Rm) - 1).max() < 1e-12


def same(a, b):
    """Two (R, info) results are the same in every bit."""
    return np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in INFO_KEYS)


def arrays(lib, mo):
    n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None
    return lib.ProblemArrays(n, ii, jj, rij)


@pytest.fixture(scope="module")
def mixed(lib):
    """The mixed batch, solved once in both modes through the public entry points; the oracle's answers."""
    from desc_amd import GCW_batch, Spectral_batch
    mos = cases.mixed_models(lib.gcw_batch_max_n())
    S = cases.mixed_S(lib.gcw_batch_max_n())
    return dict(mos=mos, S=S, gcw=GCW_batch(mos, S, return_info=True), spectral=Spectral_batch(mos, return_info=True),
                gcw_ref=[gcw_oracle(mo.Ind, mo.RijMat, s) for mo, s in zip(mos, S)],
                spectral_ref=[spectral_oracle(mo.Ind, mo.RijMat) for mo in mos])


@pytest.mark.parametrize("mode", ["gcw", "spectral"])
def test_mixed_batch_matches_dense_oracle(mixed, mode):
    for b, ((R, info), R_ref) in enumerate(zip(mixed[mode], mixed[mode + "_ref"])):
        print(mode, b, R.shape[2], info["iters"], info["products"], info["residual"], aligned_diff(R, R_ref))
    for b, ((R, info), R_ref) in enumerate(zip(mixed[mode], mixed[mode + "_ref"])):
        assert info["converged"], (b, info)
        assert_rotations(R)
        assert aligned_diff(R, R_ref) < 1e-8, (b, info)


@pytest.mark.parametrize("mode", ["gcw", "spectral"])
def test_degenerate_top_eigenspace_gives_a_consistent_answer(mode):
    """A single edge (rows == block width, spectrum +-1 three times each) and a star (row-normalised spectrum {1, 0, -1}): the top
    eigenspace is degenerate, so the oracle's basis is not a yardstick -- but on a tree every orthonormal basis of it gives rotations
    with R_i R_j' = R_ij on every edge (the dense oracle: 2.6e-15 on this star)."""
    from desc_amd import GCW_batch, Spectral_batch
    mos = [cases.single_edge(), gs.star(12, 3, seed=38)]
    if mode == "gcw":
        out = GCW_batch(mos, [gs.noisy_truth(mo, 5 + k) for k, mo in enumerate(mos)], return_info=True)
    else:
        out = Spectral_batch(mos, return_info=True)
    for mo, (R, info) in zip(mos, out):
        assert info["converged"], info
        assert_rotations(R)
        i, j = mo.Ind[:, 0] - 1, mo.Ind[:, 1] - 1
        err = np.abs(np.einsum("abe,cbe->ace", R[:, :, i], R[:, :, j]) - mo.RijMat).max()
        print(mode, R.shape[2], info["iters"], info["residual"], err)
        assert err < 1e-8, (err, info)


@pytest.mark.parametrize("mode", ["gcw", "spectral"])
def test_result_does_not_depend_on_the_batch_around_it(lib, mixed, mode):
    """As given, reversed, and each problem alone (another LDS size per launch): the same bits."""
    from desc_amd import GCW_batch, Spectral_batch
    mos, S = mixed["mos"], mixed["S"]

    def run(idx):
        if mode == "gcw":
            return GCW_batch([mos[b] for b in idx], [S[b] for b in idx], return_info=True)
        return Spectral_batch([mos[b] for b in idx], return_info=True)
    B = len(mos)
    rev = run(range(B - 1, -1, -1))
    for b in range(B):
        assert same(mixed[mode][b], rev[B - 1 - b]), b
        assert same(mixed[mode][b], run([b])[0]), b


def test_more_problems_than_compute_units(lib):
    """300 problems of 12 nodes, every one against its own 36 x 36 dense solve.  A problem whose oracle gap lambda_3 - lambda_4 is below
    1e-3 would be left out; with these seeds none is (checked on the CPU)."""
    from desc_amd import GCW_batch
    mos, S = cases.many_small(300)
    left_out = [b for b, (mo, s) in enumerate(zip(mos, S)) if cases.gcw_gap(mo, s) < 1e-3]
    print("left out:", len(left_out))
    assert len(left_out) <= 3
    out = GCW_batch(mos, S, return_info=True)
    worst = 0.0
    for b, (mo, s, (R, info)) in enumerate(zip(mos, S, out)):
        assert info["converged"], (b, info)
        assert_rotations(R)
        if b not in left_out:
            worst = max(worst, aligned_diff(R, gcw_oracle(mo.Ind, mo.RijMat, s)))
    print("worst aligned difference:", worst)
    assert worst < 1e-8


def test_empty_csr_row(lib):
    """Node 10 of 20 occurs in no edge: dinv = 0 there.  Its block is what the single GCW() call returns for it; the others agree with
    GCW() after alignment over those nodes."""
    from desc_amd import GCW, GCW_batch
    Ind, Rij, S = cases.with_empty_row()
    R, info = GCW_batch([(Ind, Rij)], [S], return_info=True)[0]
    R1 = GCW(Ind, None, Rij, S)
    assert R.shape == (3, 3, 20) and np.isfinite(R).all() and info["converged"]
    assert np.array_equal(R[:, :, 9], R1[:, :, 9])
    others = np.arange(20) != 9
    assert_rotations(R[:, :, others])
    d = aligned_diff(R[:, :, others], R1[:, :, others])
    print("empty row: block", R[:, :, 9].tolist(), "others", d)
    assert d < 1e-8


def test_desc_init_batch(lib):
    from desc_amd import DESC_PGD_batch, DESC_init, DESC_init_batch
    from desc_amd.models import Uniform_Topology
    mos = [Uniform_Topology(n, p, 0.2, 0.1, "uniform", seed=s) for n, p, s in ((12, 0.6, 51), (40, 0.5, 52), (100, 0.5, 53))]
    seeds = [3, 4, 5]
    rng = np.random.default_rng(0)
    perm = rng.permutation(mos[1].Ind.shape[0])
    problems = [mos[0], (mos[1].Ind[perm], mos[1].RijMat[:, :, perm]), mos[2]]

    def par(seed=0):
        return dict(iters=30, Gradient=ConstantStepSize(0.01), seed=seed, verbose=False, build_where=lib.BUILD_HOST)
    out = DESC_init_batch(problems, par(), seeds=seeds, return_info=True)
    S_pgd = DESC_PGD_batch(problems, par(), seeds=seeds)
    plain = DESC_init_batch(problems, par(), seeds=seeds)
    for b, (mo, (R, S_vec, info)) in enumerate(zip(mos, out)):
        assert np.array_equal(S_vec, S_pgd[b]) and np.array_equal(plain[b][1], S_vec) and np.array_equal(plain[b][0], R), b
        assert info["pgd"]["iters_run"] == 30 and info["gcw"]["converged"] and "ms_eig" in info["gcw"]["timings"], b
        S_sorted = S_vec
        if b == 1:                                   # results come back in the caller's edge order
            S_sorted = np.empty_like(S_vec); S_sorted[perm] = S_vec
        assert_rotations(R)
        d = aligned_diff(R, gcw_oracle(mo.Ind, mo.RijMat, S_sorted))
        R1, S1 = DESC_init(mo.Ind, mo.RijMat, par(seeds[b]))
        e, e1 = Rotation_Alignment(R, mo.R_orig)[2], Rotation_Alignment(R1, mo.R_orig)[2]
        print(b, d, e, e1, float(np.abs(S1 - S_sorted).max()))
        assert d < 1e-8, (b, d)
        assert abs(e - e1) < 1e-6, (b, e, e1)


def test_iteration_cap(lib):
    """max_iters = 1 on {n = 2, n = 90}: the call returns OK, the 90-node problem reports converged = 0 and valid rotations, the 2-node
    problem (its start block spans the whole space) converged = 1; neither record leaks into the other."""
    mos = [cases.single_edge(), cases.mixed_models(lib.gcw_batch_max_n())[3]]
    S = [gs.noisy_truth(mo, 9 + k) for k, mo in enumerate(mos)]
    for order in ((0, 1), (1, 0)):
        h = lib.GcwBatch([arrays(lib, mos[b]) for b in order])
        outs, _ = h.run(s_vec=np.concatenate([S[b] for b in order]), max_iters=1)
        h.destroy()
        res = {b: outs[k] for k, b in enumerate(order)}
        assert res[0][1]["converged"] and res[0][1]["iters"] == 1 and res[0][1]["products"] == 1, res[0][1]
        assert not res[1][1]["converged"] and res[1][1]["iters"] == 1 and res[1][1]["products"] > 2, res[1][1]
        assert res[1][1]["residual"] > 1e-13 >= res[0][1]["residual"]
        for b in order:
            assert_rotations(res[b][0])


def test_handle_reuse_and_a_refusal(lib, mixed):
    from desc_amd import GCW_batch
    mos = mixed["mos"][1:4]
    probs = [arrays(lib, mo) for mo in mos]
    Sa = np.concatenate(mixed["S"][1:4])
    Sb = np.concatenate([gs.noisy_truth(mo, 70 + k) for k, mo in enumerate(mos)])
    h = lib.GcwBatch(probs)
    first, again = h.run(s_vec=Sa)[0], None
    second = h.run(s_vec=Sb)[0]
    again = h.run(s_vec=Sa)[0]
    bad = Sb.copy(); bad[probs[0].m + 3] = -1.0
    with pytest.raises(lib.DescError, match=f"problem 1: S_vec holds a negative or non-finite entry \\(node {int(probs[1].ind_i[3])}\\)") as ei:
        h.run(s_vec=bad)
    assert ei.value.code == lib.ERR_INVALID
    h.destroy()
    for S, got in ((Sa, first), (Sb, second), (Sa, again)):
        f = lib.GcwBatch(probs)
        fresh = f.run(s_vec=S)[0]
        f.destroy()
        assert all(same(a, b) for a, b in zip(got, fresh))
    assert all(same(a, b) for a, b in zip(first, mixed["gcw"][1:4]))
    assert not same(first[0], second[0])
    # a refused batch launches nothing, and the next batch in the same process gives the results of the mixed test
    big = gs.band(lib.gcw_batch_max_n() + 1, 1, seed=2)
    with pytest.raises(ValueError, match="problem 1: n = "):
        GCW_batch([mixed["mos"][0], big], [mixed["S"][0], gs.noisy_truth(big, 2)])
    after = GCW_batch(mixed["mos"], mixed["S"], return_info=True)
    assert all(same(a, b) for a, b in zip(after, mixed["gcw"]))

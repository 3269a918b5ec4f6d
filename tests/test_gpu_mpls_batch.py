"""GPU tests of the batched MPLS (desc_mpls_batch_run, CempBatch.mpls_run, MPLS_batch): every problem of a batch bit for bit against
MPLS(), the sample-count classes of the H step, the bitwise independence of a problem's result from the batch around it, parity with
the NumPy oracle (the tolerances and reasons of tests/test_gpu_mpls.py: SVec 1e-12, R_init 1e-10 along the device's tree, R_est 1e-7,
score 1e-9, equal iteration counts), padded parameter vectors, handle reuse, more workgroups than compute units, permuted inputs."""
import numpy as np
import pytest

from desc_amd.algorithms import marshal_edges
from tests import mpls_batch_cases as cases

pytestmark = pytest.mark.gpu

INFO_KEYS = ("iters", "score", "cg_iters", "cg_unconverged", "cg_residual", "m_pos")


def arrays(lib, mo):
    n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None
    return lib.ProblemArrays(n, ii, jj, rij)


def single(mo, cemp, mpls, seed):
    from desc_amd import MPLS
    return MPLS(mo.Ind, mo.RijMat, dict(cemp, seed=seed), mpls, return_info=True)


def assert_equals_single(got, want, tag):
    """Entry ``got`` of MPLS_batch against MPLS(..., return_info=True): array_equal on the arrays, == on the record."""
    R_est, R_init, info = got
    R_est1, R_init1, info1 = want
    print(tag, R_est.shape[2], {k: info["mpls"][k] for k in INFO_KEYS}, {k: info1[k] for k in INFO_KEYS}, float(np.abs(R_est - R_est1).max()))
    assert np.array_equal(info["SVec"], info1["SVec"]), (tag, "SVec", float(np.abs(info["SVec"] - info1["SVec"]).max()))
    assert np.array_equal(R_init, R_init1), (tag, "R_init", float(np.abs(R_init - R_init1).max()))
    assert np.array_equal(R_est, R_est1), (tag, "R_est", float(np.abs(R_est - R_est1).max()))
    for k in INFO_KEYS:
        assert info["mpls"][k] == info1[k], (tag, k, info["mpls"][k], info1[k])


def same(a, b):
    """Two (R_est, R_init, info) entries of MPLS_batch are the same in every bit."""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2]["SVec"], b[2]["SVec"])
            and all(a[2]["mpls"][k] == b[2]["mpls"][k] for k in INFO_KEYS))


def assert_rotations(R, tol):
    Rm = np.transpose(R, (2, 0, 1))
    assert np.isfinite(Rm).all()
    assert np.abs(Rm @ np.transpose(Rm, (0, 2, 1)) - np.eye(3)).max() < tol and np.abs(np.linalg.det(Rm) - 1).max() < tol


@pytest.fixture(scope="module")
def ten(lib):
    """The ten problems, solved once through the public entry point."""
    from desc_amd import MPLS_batch
    mos = cases.models()
    cemp, mpls = cases.demo_params()
    return dict(mos=mos, cemp=cemp, mpls=mpls, out=MPLS_batch(mos, cemp, mpls, seeds=list(cases.SEEDS), return_info=True))


@pytest.mark.parametrize("max_iter", [100, 2, 3])
def test_batch_equals_the_single_call_bit_for_bit(lib, ten, max_iter):
    """max_iter = 2 is exactly one step, 3 two: a failure says whether a step or the loop control is off."""
    from desc_amd import MPLS_batch
    mos, cemp = ten["mos"], ten["cemp"]
    mpls = dict(ten["mpls"], max_iter=max_iter)
    out = ten["out"] if max_iter == 100 else MPLS_batch(mos, cemp, mpls, seeds=list(cases.SEEDS), return_info=True)
    want = [single(mo, cemp, mpls, seed) for mo, seed in zip(mos, cases.SEEDS)]
    for b, (g, w) in enumerate(zip(out, want)):
        assert_equals_single(g, w, (max_iter, b))
        assert "ms_loop" in g[2]["mpls"]["timings"] and set(g[2]) == {"SVec", "cemp", "mst", "mpls"}
    if max_iter == 100:
        assert [o[2]["mpls"]["iters"] for o in out] == list(cases.ORACLE_ITERS)
        plain = MPLS_batch(mos, cemp, mpls, seeds=list(cases.SEEDS))
        assert all(np.array_equal(p[0], o[0]) and np.array_equal(p[1], o[1]) for p, o in zip(plain, out))
    else:
        assert all(o[2]["mpls"]["iters"] == max_iter - 1 for o in out)


def test_max_iter_one_returns_the_initialisation(lib, ten):
    from desc_amd import MPLS_batch
    from oracle.refine_oracle import R2Q, q2R
    out = MPLS_batch(ten["mos"], ten["cemp"], dict(ten["mpls"], max_iter=1), seeds=list(cases.SEEDS), return_info=True)
    for b, (R_est, R_init, info) in enumerate(out):
        assert info["mpls"]["iters"] == 0 and info["mpls"]["cg_iters"] == 0
        assert np.array_equal(R_init, ten["out"][b][1])
        Q = R2Q(R_init)
        ref = np.stack([q2R(Q[i]) for i in range(Q.shape[0])], axis=2)
        assert np.abs(R_est - ref).max() < 1e-12, b          # the tolerance of test_gpu_mpls.py's test of the single call
        want = single(ten["mos"][b], ten["cemp"], dict(ten["mpls"], max_iter=1), cases.SEEDS[b])
        assert np.array_equal(R_est, want[0]), b


@pytest.mark.parametrize("nsample", cases.CLASS_NSAMPLE)
def test_sample_count_classes_equal_the_single_call(lib, nsample):
    """nsample = 70: the second lane group of cemp_edge_round's register class; 300: its two-pass class."""
    from desc_amd import MPLS_batch
    mos = [cases.models()[k] for k in cases.CLASS_PROBLEMS]
    seeds = [cases.SEEDS[k] for k in cases.CLASS_PROBLEMS]
    cemp, mpls = cases.demo_params(nsample)
    out = MPLS_batch(mos, cemp, mpls, seeds=seeds, return_info=True)
    for b, (mo, seed) in enumerate(zip(mos, seeds)):
        assert_equals_single(out[b], single(mo, cemp, mpls, seed), (nsample, b))


def test_result_does_not_depend_on_the_batch_around_it(lib, ten):
    """As given, reversed, and each problem alone (another LDS size per launch): the same bits."""
    from desc_amd import MPLS_batch
    mos = ten["mos"]

    def run(idx):
        return MPLS_batch([mos[b] for b in idx], ten["cemp"], ten["mpls"], seeds=[cases.SEEDS[b] for b in idx], return_info=True)
    B = len(mos)
    rev = run(range(B - 1, -1, -1))
    for b in range(B):
        assert same(ten["out"][b], rev[B - 1 - b]), b
        assert same(ten["out"][b], run([b])[0]), b


def test_batch_matches_the_numpy_oracle(ten):
    from tests.mpls_oracle import cemp_stage
    cemp = ten["cemp"]
    rows = []
    for b, (mo, (R_est, R_init, info)) in enumerate(zip(ten["mos"], ten["out"])):
        S = info["SVec"]
        st = cemp_stage(mo.Ind, mo.RijMat, cemp["max_iter"], cemp["reweighting"], cemp["nsample"], cases.SEEDS[b])
        ref = cases.oracle_result(b, S)
        rows.append((float(np.abs(S - st["SVec"]).max()), float(np.abs(R_init - ref["R_init"]).max()), info["mpls"]["iters"], ref["iters"],
                     float(np.abs(R_est - ref["R_est"]).max()), abs(info["mpls"]["score"] - ref["score"])))
        print(b, R_est.shape[2], rows[-1])
    for b, (dS, dR0, iters, iters_ref, dR, dscore) in enumerate(rows):
        assert dS < 1e-12, (b, dS)
        assert dR0 < 1e-10, (b, dR0)
        assert iters == iters_ref, (b, iters, iters_ref)
        assert dR < 1e-7, (b, dR)
        assert dscore < 1e-9, (b, dscore)


def test_short_parameter_vectors_are_padded(lib):
    from desc_amd import MPLS_batch
    mos = [cases.models()[k] for k in (2, 6)]
    seeds = [cases.SEEDS[k] for k in (2, 6)]
    cemp = cases.demo_params()[0]
    mpls = dict(stop_threshold=1e-4, max_iter=30, reweighting=[4.0, 8.0], thresholding=[0.9], cycle_info_ratio=[0.5, 0.25])
    out = MPLS_batch(mos, cemp, mpls, seeds=seeds, return_info=True)
    for b, (mo, seed) in enumerate(zip(mos, seeds)):
        assert_equals_single(out[b], single(mo, cemp, mpls, seed), ("padded", b))
        assert out[b][2]["mpls"]["iters"] > 2          # the loop ran past the end of every vector


def test_handle_reuse_and_refusals(lib, ten):
    cemp, mpls = ten["cemp"], ten["mpls"]
    idx = (1, 2, 3)
    probs = [arrays(lib, ten["mos"][b]) for b in idx]
    beta, tau, alpha = mpls["reweighting"], mpls["thresholding"], mpls["cycle_info_ratio"]
    h = lib.CempBatch(probs, cemp["nsample"], seeds=[cases.SEEDS[b] for b in idx])

    def rounds():
        S_list, _ = h.run(cemp["reweighting"], cemp["max_iter"])
        S = np.concatenate(S_list)
        mst, _ = lib.mst_batch_run(probs, S)
        return S, np.concatenate([R.reshape(-1, order="F") for R, _ in mst])

    def same_run(a, b):
        return np.array_equal(a[0], b[0]) and all(a[1][k] == b[1][k] for k in INFO_KEYS)
    S, R0 = rounds()
    first, tm1 = h.mpls_run(S, R0, mpls["stop_threshold"], 100, beta, tau, alpha)
    short, tm2 = h.mpls_run(S, R0, mpls["stop_threshold"], 2, beta, tau, alpha)
    assert tm1["ms_setup"] > 0 and tm2["ms_setup"] == 0
    bad = S.copy(); bad[probs[0].m + 3] = -1.0
    with pytest.raises(lib.DescError, match=f"problem 1: S_vec holds a negative or non-finite entry \\(node {int(probs[1].ind_i[3])}\\)") as ei:
        h.mpls_run(bad, R0, mpls["stop_threshold"], 100, beta, tau, alpha)
    assert ei.value.code == lib.ERR_INVALID
    Rb = R0.copy(); Rb[9 * probs[0].n + 9 * 2 + 4] = np.nan
    with pytest.raises(lib.DescError, match="problem 1: R_init holds a non-finite entry \\(node 2\\)") as ei:
        h.mpls_run(S, Rb, mpls["stop_threshold"], 100, beta, tau, alpha)
    assert ei.value.code == lib.ERR_INVALID
    with pytest.raises(lib.DescError, match="need >= 1 entry each") as ei:
        h.mpls_run(S, R0, mpls["stop_threshold"], 100, beta, [], alpha)
    assert ei.value.code == lib.ERR_INVALID
    S2, R02 = rounds()                                  # the rounds again on the same handle, then the loop again
    assert np.array_equal(S, S2) and np.array_equal(R0, R02)
    again, _ = h.mpls_run(S2, R02, mpls["stop_threshold"], 100, beta, tau, alpha)
    h.destroy()
    for k, b in enumerate(idx):
        want = ten["out"][b]
        assert same_run(first[k], again[k]), b
        assert np.array_equal(first[k][0], want[0]) and all(first[k][1][key] == want[2]["mpls"][key] for key in INFO_KEYS), b
    assert all(o[1]["iters"] == 1 for o in short) and not same_run(first[0], short[0])


def test_more_problems_than_compute_units(lib, ten):
    """300 copies of the n = 12 problem in one batch: every one is entry 1's bits."""
    from desc_amd import MPLS_batch
    mos, seeds = cases.many_small(300)
    out = MPLS_batch(mos, ten["cemp"], ten["mpls"], seeds=seeds, return_info=True)
    assert len(out) == 300
    assert all(same(o, ten["out"][1]) for o in out)


def test_permuted_double_fortran_inputs_equal_sorted(lib, ten):
    from desc_amd import MPLS_batch
    idx = (3, 7)
    items, perms = [], []
    for b in idx:
        mo = ten["mos"][b]
        perm = np.random.default_rng(b).permutation(mo.Ind.shape[0])
        items.append((mo.Ind[perm].astype(np.float64), np.asfortranarray(mo.RijMat[:, :, perm])))
        perms.append(perm)
    out = MPLS_batch(items, ten["cemp"], ten["mpls"], seeds=[cases.SEEDS[b] for b in idx], return_info=True)
    for (R_est, R_init, info), perm, b in zip(out, perms, idx):
        want = ten["out"][b]
        assert np.array_equal(R_est, want[0]) and np.array_equal(R_init, want[1]), b
        assert np.array_equal(info["SVec"], want[2]["SVec"][perm]), b
        assert np.array_equal(np.sort(perm[info["mst"]["tree_edges"]]), want[2]["mst"]["tree_edges"]), b
        assert info["mpls"]["iters"] == want[2]["mpls"]["iters"]
        # the tolerances of test_gpu_mpls.py: R_init is 3x3 products along the tree, R_est keeps the reference's unnormalised quaternions
        assert_rotations(R_init, 1e-12)
        assert_rotations(R_est, 1e-6)

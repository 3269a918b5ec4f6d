"""GPU tests of the batched refinement (desc_refine_batch_*, DESC_refine_batch, DESC_batch): every problem of a batch bit for bit against
the single call, the bitwise independence of a problem's result from the batch around it, parity with the dense oracle (the tolerances
and reasons of tests/test_gpu_refine.py: 1e-7 on the rotation entries, 1e-9 on the score, equal iteration counts), handle reuse, more
workgroups than compute units, and DESC_batch against its stages."""
import numpy as np
import pytest

from desc_amd import ConstantStepSize, Rotation_Alignment
from desc_amd.algorithms import marshal_edges
from tests import refine_batch_cases as cases

pytestmark = pytest.mark.gpu

INFO_KEYS = ("iters", "score", "cg_iters", "cg_unconverged", "cg_residual")


def arrays(lib, mo):
    n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None
    return lib.ProblemArrays(n, ii, jj, rij)


def same(a, b):
    """Two (R, info) results are the same in every bit."""
    return np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in INFO_KEYS)


def assert_rotations(R):
    Rm = np.transpose(R, (2, 0, 1))
    assert np.isfinite(Rm).all()
    assert np.abs(Rm @ np.transpose(Rm, (0, 2, 1)) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(Rm) - 1).max() < 1e-12


@pytest.fixture(scope="module")
def ten(lib):
    """The ten problems, refined once through the public entry point."""
    from desc_amd import DESC_refine_batch
    mos = cases.models()
    S, R0 = cases.inputs()
    return dict(mos=mos, S=S, R0=R0, out=DESC_refine_batch(mos, S, R0, return_info=True))


@pytest.mark.parametrize("max_iters", [100, 2, 3])
def test_batch_equals_the_single_call_bit_for_bit(lib, ten, max_iters):
    """max_iters = 2 is exactly one step, 3 two: a failure says whether a step or the loop control is off."""
    from desc_amd import DESC_refine_batch
    mos, S, R0 = ten["mos"], ten["S"], ten["R0"]
    out = ten["out"] if max_iters == 100 else DESC_refine_batch(mos, S, R0, max_iters=max_iters, return_info=True)
    single = [lib.refine_run(arrays(lib, mo), s, r, max_iters=max_iters) for mo, s, r in zip(mos, S, R0)]
    for b, ((R, info), (R1, info1)) in enumerate(zip(out, single)):
        print(max_iters, b, R.shape[2], {k: info[k] for k in INFO_KEYS}, {k: info1[k] for k in INFO_KEYS}, float(np.abs(R - R1).max()))
    for b, (got, want) in enumerate(zip(out, single)):
        assert np.array_equal(got[0], want[0]), (b, float(np.abs(got[0] - want[0]).max()))
        for k in INFO_KEYS:
            assert got[1][k] == want[1][k], (b, k, got[1][k], want[1][k])
        assert "ms_refine" in got[1]["timings"]
    if max_iters == 100:
        assert [o[1]["iters"] for o in out] == list(cases.ORACLE_ITERS)
    else:
        assert all(o[1]["iters"] == max_iters - 1 for o in out)


def test_dense_problem_equals_the_single_call_bit_for_bit(lib):
    """278 nodes at p = 0.9: the selection and the edge loops over 34.7 k edges, three steps."""
    from desc_amd import DESC_refine_batch
    mo, S, R0 = cases.dense_case()
    R, info = DESC_refine_batch([mo], [S], [R0], max_iters=4, return_info=True)[0]
    R1, info1 = lib.refine_run(arrays(lib, mo), S, R0, max_iters=4)
    print({k: info[k] for k in INFO_KEYS}, {k: info1[k] for k in INFO_KEYS}, float(np.abs(R - R1).max()))
    assert np.array_equal(R, R1)
    for k in INFO_KEYS:
        assert info[k] == info1[k], (k, info[k], info1[k])
    assert_rotations(R)


def test_result_does_not_depend_on_the_batch_around_it(lib, ten):
    """As given, reversed, and each problem alone (another LDS size per launch): the same bits."""
    from desc_amd import DESC_refine_batch
    mos, S, R0 = ten["mos"], ten["S"], ten["R0"]

    def run(idx):
        return DESC_refine_batch([mos[b] for b in idx], [S[b] for b in idx], [R0[b] for b in idx], return_info=True)
    B = len(mos)
    rev = run(range(B - 1, -1, -1))
    for b in range(B):
        assert same(ten["out"][b], rev[B - 1 - b]), b
        assert same(ten["out"][b], run([b])[0]), b


def test_batch_matches_dense_oracle(ten):
    ref = cases.oracle_results()
    for b, ((R, info), (R_ref, iters_ref, score_ref)) in enumerate(zip(ten["out"], ref)):
        print(b, R.shape[2], info["iters"], iters_ref, float(np.abs(R - R_ref).max()), abs(info["score"] - score_ref))
    for b, ((R, info), (R_ref, iters_ref, score_ref)) in enumerate(zip(ten["out"], ref)):
        assert info["iters"] == iters_ref, (b, info, iters_ref)
        assert np.abs(R - R_ref).max() < 1e-7, (b, np.abs(R - R_ref).max())
        assert abs(info["score"] - score_ref) < 1e-9, b


def test_handle_run_twice_and_a_refusal(lib, ten):
    mos = ten["mos"][1:4]
    probs = [arrays(lib, mo) for mo in mos]
    S = np.concatenate(ten["S"][1:4])
    R0 = np.concatenate([r.reshape(-1, order="F") for r in ten["R0"][1:4]])
    h = lib.RefineBatch(probs)
    first = h.run(S, R0)[0]
    short = h.run(S, R0, max_iters=2)[0]
    bad = S.copy(); bad[probs[0].m + 3] = -1.0
    with pytest.raises(lib.DescError, match=f"problem 1: S_vec holds a negative or non-finite entry \\(node {int(probs[1].ind_i[3])}\\)") as ei:
        h.run(bad, R0)
    assert ei.value.code == lib.ERR_INVALID
    Rb = R0.copy(); Rb[9 * probs[0].n + 9 * 2 + 4] = np.nan
    with pytest.raises(lib.DescError, match="problem 1: R_init holds a non-finite entry \\(node 2\\)") as ei:
        h.run(S, Rb)
    assert ei.value.code == lib.ERR_INVALID
    again = h.run(S, R0)[0]
    h.destroy()
    assert all(same(a, b) for a, b in zip(first, again))
    assert all(same(a, b) for a, b in zip(first, ten["out"][1:4]))
    assert all(o[1]["iters"] == 1 for o in short) and not same(first[0], short[0])


def test_more_problems_than_compute_units(lib, ten):
    """300 copies of the n = 12 problem in one batch: every one is entry 1's bits."""
    from desc_amd import DESC_refine_batch
    mos, S, R0 = cases.many_small(300)
    out = DESC_refine_batch(mos, S, R0, return_info=True)
    assert len(out) == 300
    assert all(same(o, ten["out"][1]) for o in out)


def test_desc_batch(lib):
    from desc_amd import DESC_batch, DESC_init_batch, DESC_refine_batch
    from desc_amd.models import Uniform_Topology
    from oracle.refine_oracle import desc_refine_oracle
    mos = [Uniform_Topology(60, 0.5, q, 0.1, "uniform", seed=t) for t, q in enumerate((0.1, 0.3, 0.1, 0.3, 0.1, 0.3))]
    par = dict(iters=50, Gradient=ConstantStepSize(0.01), learning_rate=0.01, verbose=True, build_where=lib.BUILD_HOST)
    out = DESC_batch(mos, par, return_info=True)
    plain = DESC_batch(mos, par)
    init = DESC_init_batch(mos, par)
    ref = DESC_refine_batch(mos, [s for _, s in init], [r for r, _ in init], return_info=True)
    for b, (mo, (R_est, R_init, S_vec, info)) in enumerate(zip(mos, out)):
        assert np.array_equal(S_vec, init[b][1]) and np.array_equal(R_init, init[b][0]), b
        assert np.array_equal(R_est, ref[b][0]), b
        assert all(np.array_equal(x, y) for x, y in zip(plain[b], (R_est, R_init, S_vec))), b
        assert set(info) == {"pgd", "gcw", "refine"} and info["refine"]["iters"] == ref[b][1]["iters"] and "ms_refine" in info["refine"]["timings"]
        assert info["pgd"]["iters_run"] == 50 and info["gcw"]["converged"], b
        assert_rotations(R_est)
        R_ref, iters_ref, _ = desc_refine_oracle(mo.Ind, mo.RijMat, S_vec, R_init)
        e, e_ref = Rotation_Alignment(R_est, mo.R_orig)[2], Rotation_Alignment(R_ref, mo.R_orig)[2]
        print(b, info["refine"]["iters"], iters_ref, e, e_ref, Rotation_Alignment(R_init, mo.R_orig)[2])
        assert abs(e - e_ref) < 1e-6, (b, e, e_ref)

"""GPU tests of the batched IRLS (IRLS_GM_batch / IRLS_L12_batch, desc_irls_batch_*): every entry is bit for bit the single call's --
R, R_l1 and every count and score of the record -- whatever the batch around it.  The tolerance is zero: both paths run the same
per-element text (csrc/irls_math.h, csrc/laa_math.h) and take every sum in the same order, with contraction off.  One problem is also
held against the NumPy / SciPy restatement (tests/irls_oracle.py), so that the two device paths cannot be wrong together."""
import warnings

import numpy as np
import pytest

from desc_amd import IRLS_GM_batch, IRLS_L12_batch, _lib
from tests import irls_batch_cases as cases

pytestmark = pytest.mark.gpu

BATCH = {"GM": IRLS_GM_batch, "L12": IRLS_L12_batch}
KEYS = ("l1_iters", "irls_iters", "l1_score", "irls_score", "pd_steps", "pd_ill", "pd_stuck", "pd_solves", "cg_iters_l1", "cg_iters_irls",
        "cg_unconverged", "cg_residual", "warned_edges", "comp_nodes", "comp_edges")


def assert_same(got, want, what=""):
    (R, info), (R_s, info_s) = got, want
    assert np.array_equal(R, R_s), what
    assert np.array_equal(info["R_l1"], info_s["R_l1"]), what
    for k in KEYS:
        assert info[k] == info_s[k], (what, k, info[k], info_s[k])


def batch_result(mode, MaxIterations=(10, 100)):
    """The ten case problems in one call: once per process."""
    return cases._once(("batch", mode, tuple(MaxIterations)),
                       lambda: BATCH[mode](cases.problems(), MaxIterations=MaxIterations, return_info=True))


@pytest.mark.parametrize("mode", ["GM", "L12"])
@pytest.mark.parametrize("MaxIterations", [(10, 100), (1, 1), (2, 3)], ids=["full", "one-step", "two-three"])
def test_bit_for_bit_against_the_single_call(mode, MaxIterations):
    outs = batch_result(mode, MaxIterations)
    assert len(outs) == len(cases.problems())
    for k, got in enumerate(outs):
        assert_same(got, cases.single(mode, k, MaxIterations), f"problem {k}")
        assert set(got[1]) == {*KEYS, "R_l1", "timings"}                                # the stage times are the batch's
        assert set(got[1]["timings"]) == {"ms_structure", "ms_upload", "ms_project", "ms_solve", "ms_total"}
    if MaxIterations == (10, 100):
        for k, (_args, m, l1, gm, l12, pd) in enumerate(cases.TABLE):
            info = outs[k][1]
            assert info["comp_edges"] == m
            assert (info["l1_iters"], info["irls_iters"], info["pd_steps"]) == (l1, gm if mode == "GM" else l12, pd), (k, info)
            assert info["pd_ill"] == info["pd_stuck"] == info["warned_edges"] == info["cg_unconverged"] == 0
    if MaxIterations == (1, 1):
        for _, info in outs:
            assert info["l1_iters"] == 1 and info["irls_iters"] == 1 and info["pd_solves"] <= 2


@pytest.mark.parametrize("mode", ["GM", "L12"])
def test_no_bit_depends_on_the_batch_around_a_problem(mode):
    """The batch as given, reversed, and each problem alone (another LDS size for all but the largest)."""
    outs = batch_result(mode)
    rev = BATCH[mode](cases.problems()[::-1], return_info=True)[::-1]
    for k, (a, b) in enumerate(zip(outs, rev)):
        assert_same(b, a, f"reversed, problem {k}")
    for k in range(len(cases.problems())):
        alone = BATCH[mode]([cases.problems()[k]], return_info=True)
        assert_same(alone[0], outs[k], f"alone, problem {k}")
    plain = BATCH[mode](cases.problems())
    assert all(np.array_equal(R, o[0]) for R, o in zip(plain, outs))


@pytest.mark.parametrize("mode", ["GM", "L12"])
def test_shuffled_rows_follow_the_caller_s_order(mode):
    """Shuffled Ind rows change the caller's order and with it the spanning-tree start: the batch follows the single call on the same
    arrays, and R_l1 is not the unshuffled problem's."""
    ks = (1, 2, 4)
    probs = [cases.shuffled(k) for k in ks]
    outs = BATCH[mode](probs, return_info=True)
    differs = 0
    for k, pair, got in zip(ks, probs, outs):
        assert_same(got, cases.single(mode, pair), f"shuffled problem {k}")
        differs += not np.array_equal(got[1]["R_l1"], cases.single(mode, k)[1]["R_l1"])
    assert differs >= 1


@pytest.mark.parametrize("mode", ["GM", "L12"])
def test_projection_warnings_and_the_error_s_row(mode):
    P = cases.problems()
    Ind1, R1 = P[1]
    scaled = R1.copy()
    scaled[:, :, [5, 40, 100]] *= 1.03
    with pytest.warns(RuntimeWarning, match=r"problems 1 \(3\)$") as rec:
        outs = BATCH[mode]([P[0], (Ind1, scaled), P[2]], return_info=True)
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1        # one line for the batch
    assert [o[1]["warned_edges"] for o in outs] == [0, 3, 0]
    assert_same(outs[1], cases.single(mode, (Ind1, scaled)), "scaled blocks")
    assert_same(outs[0], cases.single(mode, 0)); assert_same(outs[2], cases.single(mode, 2))
    # a block with negated determinant in problem 2, at a known caller row of its shuffled Ind; a later one in problem 3
    Ind2, R2 = cases.shuffled(2)
    bad2 = R2.copy(); bad2[:, :, 77] = -bad2[:, :, 77]; bad2[:, :, 300] = -bad2[:, :, 300]
    Ind3, R3 = P[3]
    bad3 = R3.copy(); bad3[:, :, 4] = -bad3[:, :, 4]
    with pytest.raises(_lib.DescError, match=r"problem 2: det\(RR\(:,:,78\)\)=-1\.0") as ei:
        BATCH[mode]([P[0], P[1], (Ind2, bad2), (Ind3, bad3)])
    assert ei.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.DescError, match=r"det\(RR\(:,:,78\)\)=-1\.0") as es:      # the single call's numbers
        cases.single(mode, (Ind2, bad2))
    assert str(ei.value).replace("problem 2: ", "", 1) == str(es.value)
    # all three singular values off 1 by >= 0.1
    big = R1.copy(); big[:, :, 9] *= 1.2
    with pytest.raises(_lib.DescError, match=r"problem 0: svd\(RR\(:,:,10\)\)=\[1\.2"):
        BATCH[mode]([(Ind1, big)])


@pytest.mark.parametrize("mode", ["GM", "L12"])
def test_degenerate_coordinates_take_the_ill_conditioned_return_of_the_single_call(mode):
    """Rotations about one axis: two coordinates of every edge's log map are zero, which l1decode_pd cannot solve (u = 0, a division by
    zero).  The single call ends such a coordinate by a tracked PCG breakdown ("Matrix ill-conditioned": pd_ill = 20 here, two
    coordinates in each of the ten L1 iterations; pd_stuck stays 0, so pd_trial's 32-trial limit is not reached by this case).  The
    workgroup takes the same early returns through wg_pcg<true, true>'s breakdown tracking and gives the same bits, next to ordinary
    problems in the same batch."""
    pair = cases.planar()
    outs = BATCH[mode]([cases.problems()[0], pair, cases.problems()[1]], return_info=True)
    (R, info), (R_s, info_s) = outs[1], cases.single(mode, pair)
    assert info_s["pd_ill"] > 0, info_s                                      # the case does what it is here for
    assert np.array_equal(R, R_s, equal_nan=True) and np.array_equal(info["R_l1"], info_s["R_l1"], equal_nan=True)
    for k in KEYS:
        assert np.array_equal(info[k], info_s[k], equal_nan=True), (k, info[k], info_s[k])
    assert_same(outs[0], cases.single(mode, 0)); assert_same(outs[2], cases.single(mode, 1))


def test_one_handle_runs_gm_then_l12():
    from desc_amd.algorithms import _marshal_problems
    probs, perms = _marshal_problems(cases.problems()[:4] + [cases.shuffled(2)])
    h = _lib.IrlsBatch(probs, perms)
    try:
        for mode, const in (("GM", _lib.IRLS_GM), ("L12", _lib.IRLS_L12), ("GM", _lib.IRLS_GM)):
            outs, timings = h.run(const)
            assert timings["ms_solve"] > 0
            for k, (R, R_l1, info) in enumerate(outs[:4]):
                Rb, ib = batch_result(mode)[k]
                assert np.array_equal(R, Rb) and np.array_equal(R_l1, ib["R_l1"]) and all(info[key] == ib[key] for key in KEYS)
            assert_same((outs[4][0], dict(outs[4][2], R_l1=outs[4][1])), cases.single(mode, cases.shuffled(2)))
    finally:
        h.destroy()


def test_more_workgroups_than_compute_units():
    outs = IRLS_GM_batch([cases.problems()[0]] * 300, return_info=True)
    assert len(outs) == 300
    assert_same(outs[0], cases.single("GM", 0))
    for R, info in outs[1:]:
        assert np.array_equal(R, outs[0][0]) and np.array_equal(info["R_l1"], outs[0][1]["R_l1"])
        assert all(info[k] == outs[0][1][k] for k in KEYS)


@pytest.mark.parametrize("mode", ["GM", "L12"])
def test_oracle_parity(mode):
    """The 30-node problem of tests/test_gpu_irls.py from the batch against the restatement, with that file's tolerances."""
    from tests.irls_oracle import irls_oracle
    Ind, Rij = cases.problems()[cases.ORACLE_CASE]
    R, info = batch_result(mode)[cases.ORACLE_CASE]
    ref, ref1, tr = cases._once(("oracle", mode), lambda: irls_oracle(Rij, Ind, mode))
    assert info["l1_iters"] == tr["l1_iters"] and info["irls_iters"] == tr["irls_iters"]
    assert (info["pd_steps"], info["pd_ill"], info["pd_stuck"]) == (tr["steps"], tr["ill"], tr["stuck"])
    assert info["comp_nodes"] == tr["comp_nodes"] and info["comp_edges"] == tr["comp_edges"] and info["warned_edges"] == tr["warned"]
    assert info["cg_unconverged"] == 0
    d1, d = float(np.abs(info["R_l1"] - ref1).max()), float(np.abs(R - ref).max())
    print(f"oracle parity {mode}: |R_l1 - ref| = {d1:.3e}, |R - ref| = {d:.3e}")
    assert d1 <= 1e-9, d1
    assert d <= 1e-7, d


def test_warning_free_batches_warn_about_nothing():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        IRLS_GM_batch(cases.problems()[:2], MaxIterations=(1, 1))

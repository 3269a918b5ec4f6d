"""CPU tests (no GPU, no launch) of the inputs of tests/test_gpu_batch_caps.py (tests/batch_cap_cases.py), so that a failure on the GPU
means the kernel and not the case: every problem sits where it is meant to relative to the cap the library reports, is connected and
touches every node id; the restatements do not sit on their stop rules; the PGD structures have the full lane groups they are there
for; the bytes of LDS each launch declares at its cap stay within what one workgroup may declare.

The refusals of cap + 1 are tested where the calls are (tests/test_refine_batch_host.py, test_mpls_batch_host.py, test_irls_batch_host.py,
test_cemp_batch_host.py and test_lp_batch_host.py, the last two also for a CSR row of cap + 1 entries)."""
import numpy as np
import pytest

from tests import batch_cap_cases as cases
from tests import cemp_batch_cases
from tests import graph_shapes as gs


def whole(Ind, n):
    return int(np.asarray(Ind).max()) == n and int(np.asarray(Ind).min()) == 1 and cases.connected(Ind) and np.unique(Ind).size == n


def test_every_problem_sits_at_its_cap_and_is_connected(lib):
    cap = cases.caps()
    assert cap == dict(refine=lib.refine_batch_max_n(), mpls=lib.mpls_batch_max_n(), irls=lib.irls_batch_max_n(), mst=lib.mst_batch_max_n(),
                       row=lib.cemp_batch_max_degree())
    assert cap["mpls"] == cap["refine"] > 513 and cap["irls"] > 513          # the third block of 256 rows lies below every cap
    for mo, n in ((cases.laa_cap(), cap["refine"]), (cases.laa_cap_minus_one(), cap["refine"] - 1), (cases.laa_n513(), 513)):
        assert whole(mo.Ind, n), n
    for (Ind, _), n in ((cases.irls_cap(), cap["irls"]), (cases.irls_n513(), 513)):
        assert whole(Ind, n), n
    items = cases.mst_cap()
    assert [name.split("-")[0] for name, _, _ in items] == ["path"] * 4 + ["star1"] * 4 + ["star%d" % cap["mst"]] * 4 + ["er"]
    for name, mo, S in items:
        assert whole(mo.Ind, cap["mst"]) and S.shape == (mo.Ind.shape[0],) and np.isfinite(S).all(), name
    assert gs.degrees(items[4][1].Ind)[0] == cap["mst"] - 1 and gs.degrees(items[8][1].Ind)[-1] == cap["mst"] - 1
    for hub_id in (2000, 1, -1):
        mo = cases.row_cap(hub_id)
        d = np.sort(gs.degrees(mo.Ind))
        want = cap["row"] + 1 if hub_id == -1 else hub_id
        assert whole(mo.Ind, cap["row"] + 1) and int(np.argmax(gs.degrees(mo.Ind))) + 1 == want, hub_id
        assert d[-1] == cap["row"] and d[-2] < 64 and d[0] >= 2, (hub_id, d[-3:], d[0])      # exactly the longest row the sampler stages
        assert cases.hub_edges(mo, want).size == cap["row"]
    if cap == dict(refine=748, mpls=748, irls=557, mst=4096, row=4096):       # the figures of tests/batch_cap_cases.py's docstring
        assert cases.laa_cap().Ind.shape[0] == 4496 and cases.irls_cap()[0].shape[0] == 3420 and cases.row_cap().Ind.shape[0] == 24991
        d = np.sort(gs.degrees(cases.row_cap().Ind))
        assert (d[-2], d[0]) == (24, 4)


def test_declared_lds_at_the_caps(lib):
    """The bytes a launch at the cap declares: 26 doubles per node next to the 8 KiB set aside for the fixed LDS of k_refine_batch and
    k_mpls_batch (csrc/laa_wg.h), 34 per node next to 12 KiB for k_irls_batch (csrc/irls_batch.hip), within the 160 KiB one workgroup may
    declare on gfx950; 16 bytes per node of the tree kernel and 4 waves x 4 bytes per staged row position within 64 KiB."""
    cap = cases.caps()
    assert 8 * 26 * cap["refine"] + 8 * 1024 <= 160 * 1024 and 8 * 26 * cap["mpls"] + 8 * 1024 <= 160 * 1024
    assert 8 * 34 * cap["irls"] + 12 * 1024 <= 160 * 1024
    assert 16 * cap["mst"] <= 64 * 1024 and 4 * 4 * cap["row"] <= 64 * 1024
    if cap["refine"] == 748 and cap["irls"] == 557:
        assert (8 * 26 * cap["refine"], 8 * 34 * cap["irls"]) == (155584, 151504)


def off_rotation(R):
    Rm = np.transpose(R, (2, 0, 1))
    return max(float(np.abs(Rm @ np.transpose(Rm, (0, 2, 1)) - np.eye(3)).max()), float(np.abs(np.linalg.det(Rm) - 1).max()))


def test_refinement_oracle_is_well_conditioned_at_the_cap():
    """The same iteration count with the threshold moved by +-0.1 % (as tests/refine_batch_cases.py documents for its problems).  And
    the oracle's own result is a rotation to half the 1e-12 the device's is held to: the reference keeps the unnormalised quaternions
    of Utils/R2Q.m, which is ill-conditioned at a start that turns by nearly pi (tests/batch_cap_cases.py: seed 61), and the oracle and
    the device round that start independently."""
    its = [cases.refine_oracle_result(th)[1] for th in (1e-3, 0.999e-3, 1.001e-3)]
    R_ref, _, score = cases.refine_oracle_result()
    print(its, score, off_rotation(R_ref))
    assert its == [cases.REFINE_ITERS] * 3 and cases.REFINE_ITERS >= 4
    assert abs(score - 9.77e-4) < 0.01e-4
    assert off_rotation(R_ref) <= 0.5e-12
    from tests import refine_batch_cases
    assert off_rotation(refine_batch_cases.oracle_results()[cases.LAA_SMALL][0]) <= 0.5e-12      # the small problem at its side


def test_mpls_oracle_does_not_sit_on_its_stop_rule_at_the_cap():
    """No step's score lies within 0.1 % of stop_threshold: the iteration count is the same with the threshold moved by +-0.1 % (one run
    instead of three; tests/test_gpu_batch_caps.py asserts the same of the run on the device's tree)."""
    ref = cases.mpls_oracle_result()
    print(ref["iters"], ref["scores"][-3:])
    assert ref["iters"] == len(ref["scores"]) == cases.MPLS_ITERS >= 4
    assert cases.stop_is_clear(ref["scores"], 1e-3)


def test_irls_oracle_is_well_conditioned_at_the_cap():
    """One ulp of RijMat moves the restatement by at most 1/100 of what the device is held to (1e-9 in R_l1, 1e-7 in R) and leaves its
    counts alone: the rule of tests/test_graph_shapes.py."""
    from tests.irls_oracle import irls_oracle
    Ind, Rij = cases.irls_cap()
    R, R1, tr = irls_oracle(Rij, Ind, "GM")
    Rp, R1p, trp = irls_oracle(gs.ulp_perturbed(Rij, 1), Ind, "GM")
    d1, d = float(np.abs(R1 - R1p).max()), float(np.abs(R - Rp).max())
    print(tr["l1_iters"], tr["irls_iters"], tr["steps"], d1, d)
    assert (tr["l1_iters"], tr["irls_iters"], tr["steps"], tr["ill"], tr["stuck"], tr["warned"]) == (10, 23, 60, 0, 0, 0)
    assert (trp["l1_iters"], trp["irls_iters"], trp["steps"]) == (tr["l1_iters"], tr["irls_iters"], tr["steps"])
    assert d1 <= 1e-11 and d <= 1e-9


@pytest.mark.parametrize("hub_id", [2000, 1, -1])
def test_cemp_oracle_is_well_conditioned_at_the_longest_row(hub_id):
    """One ulp of RijMat moves cemp_oracle_batched by at most a tenth of the 1e-12 the device is held to.  (tests/test_graph_shapes.py
    asks 1/100 of its shapes, of at most 8300 nodes with 3e-15 .. 8e-15 of movement; the six reweighting rounds amplify more on these
    25 000 edges: 1.1e-14, 1.0e-14 and 1.6e-14.)"""
    from oracle.cemp_oracle import cemp_oracle_batched
    mo = cases.row_cap(hub_id)
    S = cemp_oracle_batched(mo.Ind, mo.RijMat, 6, cemp_batch_cases.BETA, 50, 1)
    d = max(float(np.abs(S - cemp_oracle_batched(mo.Ind, gs.ulp_perturbed(mo.RijMat, s), 6, cemp_batch_cases.BETA, 50, 1)).max()) for s in (1, 2))
    print(hub_id, d)
    assert d <= 1e-13


def test_sampling_restatement_for_single_edges_is_cemp_stage_s():
    """cases.sampled_edges_oracle against tests/mpls_oracle.py: cemp_stage on the 300-node hub graph of tests/cemp_batch_cases.py."""
    from tests.mpls_oracle import cemp_stage
    mo = cemp_batch_cases.model("hub300")
    st = cemp_stage(mo.Ind, mo.RijMat, 0, cemp_batch_cases.BETA, 50, 1)
    e_jk, e_ki = cases.sampled_edges_oracle(mo.Ind, np.arange(mo.Ind.shape[0]), 50, 1)
    P = st["IndPosbin"]
    assert P.sum() > 299 and np.array_equal(e_jk[P], st["Ejk"].T[P]) and np.array_equal(e_ki[P], st["Eki"].T[P])
    assert (e_jk[~P] == -1).all() and (e_ki[~P] == -1).all()


@pytest.mark.parametrize("T", cases.PGD_T)
def test_pgd_structures_have_full_lane_groups(oracle, T):
    """n_sample == T and a longest segment == T on the problem the T is run on; at T = 64 at least 3000 segments of exactly 64."""
    which = "mid" if T < cases.PGD_DENSE_MIN_T else "dense"
    q = {"mid": cases.pgd_mid, "dense": cases.pgd_dense}[which]()
    st = oracle.build_structure(q["n"], q["ii"], q["jj"], seed=cases.PGD_SEED, n_sample_min=T)
    seg = np.diff(st["cum_ind"])
    assert st["n_sample"] == T and int(seg.max()) == T, (which, st["n_sample"], int(seg.max()))
    if T <= 33:
        assert (seg == T).all()
    if T == 64:
        assert int((seg == 64).sum()) >= 3000
    sp = cases.pgd_sparse()
    st = oracle.build_structure(sp["n"], sp["ii"], sp["jj"], seed=cases.PGD_SEED, n_sample_min=T)
    assert st["n_sample"] == T and int(np.diff(st["cum_ind"]).max()) == 5


def test_pgd_dense_is_the_graph_it_is_described_as():
    cd = gs.codegrees(cases.pgd_dense()["mo"].Ind)
    assert (cd.size, cd.min(), cd.max(), np.median(cd)) == (3599, 60, 82, 71) and int(np.ceil(np.median(cd) / 4)) == cases.PGD_DENSE_MIN_T
    assert (cd >= 64).mean() > 0.98
    cd = gs.codegrees(cases.pgd_mid()["mo"].Ind)
    assert (cd.size, cd.min(), cd.max(), np.median(cd)) == (3212, 41, 71, 57) and int(np.ceil(np.median(cd) / 4)) <= 16

"""GPU tests of every batched call at the largest size its create call accepts (tests/batch_cap_cases.py; the inputs are qualified on
the CPU by tests/test_batch_caps_host.py): the launch with the most dynamic LDS a call may ask for, the third block of 256 rows of the
Lie-algebraic averaging core, a tree of 4096 nodes, a CSR row of 4096 entries under the sampler's staging, and segments that fill the
16-, 32- and 64-lane groups of the batched sweep.

Every tolerance is an existing one, named where it is used by the file it comes from.  The CPU restatements are computed once per
process (tests/batch_cap_cases.py: _once) and left unchanged."""
import numpy as np
import pytest

from desc_amd.algorithms import marshal_edges
from tests import batch_cap_cases as cases
from tests import cemp_batch_cases, irls_batch_cases, mpls_batch_cases, refine_batch_cases
from tests.helpers import assert_structure_equal, c_params
from tests.mpls_oracle import kruskal, propagate

pytestmark = pytest.mark.gpu


def arrays(lib, mo):
    n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None
    return lib.ProblemArrays(n, ii, jj, rij)


# ---- the refinement at n = 748 ---------------------------------------------------------------------------------------------------
def refine_problems():
    """name -> (model, S, R_init)."""
    def make():
        cap, minus, n513 = cases.laa_cap(), cases.laa_cap_minus_one(), cases.laa_n513()
        return dict(small=cases.laa_small(), cap=(cap,) + cases.laa_cap_inputs(), minus=(minus,) + cases.turned_truth_inputs(minus, 362),
                    n513=(n513,) + cases.turned_truth_inputs(n513, 363))
    return cases._once("refine_problems", make)


def refine_single(lib, name):
    mo, S, R0 = refine_problems()[name]
    return cases._once(("refine_single", name), lambda: lib.refine_run(arrays(lib, mo), S, R0))


def refine_batch(names):
    from desc_amd import DESC_refine_batch
    P = refine_problems()
    return DESC_refine_batch([P[k][0] for k in names], [P[k][1] for k in names], [P[k][2] for k in names], return_info=True)


@pytest.mark.parametrize("names", [("small", "cap"), ("cap", "small"), ("cap",), ("minus", "n513", "cap")], ids="-".join)
def test_refine_at_the_cap_equals_the_single_call_bit_for_bit(lib, names):
    """The comparison of tests/test_gpu_refine_batch.py::test_batch_equals_the_single_call_bit_for_bit; every composition is compared
    with the same single results, so the compositions agree among themselves."""
    from tests.test_gpu_refine_batch import INFO_KEYS, assert_rotations
    assert int(refine_problems()["cap"][0].Ind.max()) == lib.refine_batch_max_n()
    for k, (R, info) in zip(names, refine_batch(names)):
        R1, info1 = refine_single(lib, k)
        Rm = np.transpose(R, (2, 0, 1))
        print(names, k, R.shape[2], {key: info[key] for key in INFO_KEYS}, {key: info1[key] for key in INFO_KEYS}, float(np.abs(R - R1).max()),
              "off a rotation by", float(np.abs(Rm @ np.transpose(Rm, (0, 2, 1)) - np.eye(3)).max()))
        assert np.array_equal(R, R1), (k, float(np.abs(R - R1).max()))
        for key in INFO_KEYS:
            assert info[key] == info1[key], (k, key, info[key], info1[key])
        assert info["iters"] >= 2 and info["cg_unconverged"] == 0, (k, info)
        assert_rotations(R)                                  # 1e-12, as there


def test_refine_at_the_cap_matches_the_dense_oracle(lib):
    """tests/test_gpu_refine_batch.py::test_batch_matches_dense_oracle's bounds: 1e-7 on the rotation entries, 1e-9 on the score, equal
    iteration counts (19: tests/test_batch_caps_host.py)."""
    R, info = refine_batch(("cap",))[0]
    R_ref, iters_ref, score_ref = cases.refine_oracle_result()
    print(info["iters"], iters_ref, float(np.abs(R - R_ref).max()), abs(info["score"] - score_ref))
    assert info["iters"] == iters_ref == cases.REFINE_ITERS
    assert np.abs(R - R_ref).max() < 1e-7
    assert abs(info["score"] - score_ref) < 1e-9


def test_small_launch_after_the_largest_one_gives_the_same_bits(lib):
    """The kernel's dynamic-LDS attribute is raised to the cap's and never lowered: a handle at the cap run twice, then a handle of
    small problems, whose bits are those they had before the large launch."""
    from tests.test_gpu_refine_batch import same
    mos = refine_batch_cases.models()[1:4]
    S, R0 = refine_batch_cases.inputs()
    Sc = np.concatenate(S[1:4])
    R0c = np.concatenate([r.reshape(-1, order="F") for r in R0[1:4]])

    def small_run():
        h = lib.RefineBatch([arrays(lib, mo) for mo in mos])
        try:
            return h.run(Sc, R0c)[0]
        finally:
            h.destroy()
    before = small_run()
    mo, Scap, Rcap = refine_problems()["cap"]
    h = lib.RefineBatch([arrays(lib, mo)])
    try:
        first = h.run(Scap, Rcap.reshape(-1, order="F"))[0]
        second = h.run(Scap, Rcap.reshape(-1, order="F"))[0]
    finally:
        h.destroy()
    after = small_run()
    assert same(first[0], second[0]) and same(first[0], refine_single(lib, "cap"))
    for b, (x, y) in enumerate(zip(before, after)):
        assert same(x, y), b
        assert same(x, lib.refine_run(arrays(lib, mos[b]), S[1 + b], R0[1 + b])), b


# ---- MPLS at n = 748 -------------------------------------------------------------------------------------------------------------
def mpls_batch(order):
    """MPLS_batch on the n = 40 problem of mpls_batch_cases and laa_cap(), in the given order -> name -> entry."""
    def make():
        from desc_amd import MPLS_batch
        P = dict(small=(mpls_batch_cases.models()[2], mpls_batch_cases.SEEDS[2]), cap=(cases.laa_cap(), cases.MPLS_SEED))
        cemp, mpls = mpls_batch_cases.demo_params()
        out = MPLS_batch([P[k][0] for k in order], cemp, mpls, seeds=[P[k][1] for k in order], return_info=True)
        return dict(zip(order, out))
    return cases._once(("mpls_batch", order), make)


@pytest.mark.parametrize("order", [("small", "cap"), ("cap", "small")], ids="-".join)
def test_mpls_at_the_cap_equals_the_single_call_bit_for_bit(lib, order):
    from tests.test_gpu_mpls_batch import assert_equals_single, single
    cemp, mpls = mpls_batch_cases.demo_params()
    out = mpls_batch(order)
    assert out["cap"][0].shape[2] == lib.mpls_batch_max_n()
    want = dict(small=cases._once("mpls_single_small", lambda: single(mpls_batch_cases.models()[2], cemp, mpls, mpls_batch_cases.SEEDS[2])),
                cap=cases._once("mpls_single_cap", lambda: single(cases.laa_cap(), cemp, mpls, cases.MPLS_SEED)))
    for k in order:
        assert_equals_single(out[k], want[k], (order, k))
    assert out["cap"][2]["mpls"]["cg_unconverged"] == 0


def test_mpls_at_the_cap_matches_the_numpy_oracle(lib):
    """tests/test_gpu_mpls_batch.py::test_batch_matches_the_numpy_oracle's bounds: SVec 1e-12, R_init 1e-10 along the device's tree,
    R_est 1e-7, score 1e-9, equal iteration counts.  The oracle builds its tree from the device's SVec, as there: two edges of a triangle
    that is the only cycle of both carry the same SVec up to round-off, and which of them the tree takes decides the start (and the
    iteration count: 30 on the device's tree, 26 on the oracle's own; 94 pairs of the oracle's keys differ by less than 1e-13)."""
    R_est, R_init, info = mpls_batch(("small", "cap"))["cap"]
    ref = cases.mpls_oracle_result(info["SVec"])
    row = (float(np.abs(info["SVec"] - ref["SVec"]).max()), float(np.abs(R_init - ref["R_init"]).max()), info["mpls"]["iters"], ref["iters"],
           float(np.abs(R_est - ref["R_est"]).max()), abs(info["mpls"]["score"] - ref["score"]))
    print(R_est.shape[2], row)
    dS, dR0, iters, iters_ref, dR, dscore = row
    assert dS < 1e-12 and dR0 < 1e-10
    assert iters == iters_ref >= 4
    assert cases.stop_is_clear(ref["scores"], 1e-3), ref["scores"][-3:]      # on the device's tree too, no step lies within 0.1 % of the stop rule
    assert dR < 1e-7 and dscore < 1e-9


# ---- IRLS at n = 557 -------------------------------------------------------------------------------------------------------------
IRLS_NAMES = ("small", "n513", "cap")


def irls_problem(name):
    return dict(small=lambda: irls_batch_cases.problems()[0], n513=cases.irls_n513, cap=cases.irls_cap)[name]()


def irls_single(mode, name, MaxIterations):
    return cases._once(("irls_single", mode, name, MaxIterations), lambda: irls_batch_cases.single(mode, irls_problem(name), MaxIterations))


@pytest.mark.parametrize("MaxIterations", [(10, 100), (1, 1)], ids=["full", "one-step"])
@pytest.mark.parametrize("mode", ["GM", "L12"])
def test_irls_at_the_cap_equals_the_single_call_bit_for_bit(lib, mode, MaxIterations):
    """As given and reversed; R, R_l1 and every key of tests/test_gpu_irls_batch.py: KEYS."""
    from tests.test_gpu_irls_batch import BATCH, assert_same
    assert int(cases.irls_cap()[0].max()) == lib.irls_batch_max_n()
    for names in (IRLS_NAMES, IRLS_NAMES[::-1]):
        outs = BATCH[mode]([irls_problem(k) for k in names], MaxIterations=MaxIterations, return_info=True)
        for k, got in zip(names, outs):
            print(mode, MaxIterations, names, k, {key: got[1][key] for key in ("l1_iters", "irls_iters", "pd_steps", "cg_unconverged")})
            assert_same(got, irls_single(mode, k, MaxIterations), (mode, names, k))
    if MaxIterations == (10, 100):
        info = outs[0][1]                                # the cap, first in the reversed batch
        assert info["comp_nodes"] == lib.irls_batch_max_n() and info["pd_ill"] == info["pd_stuck"] == info["warned_edges"] == info["cg_unconverged"] == 0


def test_irls_at_the_cap_matches_the_restatement(lib):
    """GM mode at MaxIterations = (10, 100) against tests/irls_oracle.py with tests/test_gpu_irls_batch.py::test_oracle_parity's bounds:
    1e-9 in R_l1, 1e-7 in R, equal counts."""
    from desc_amd import IRLS_GM_batch
    from tests.irls_oracle import irls_oracle
    Ind, Rij = cases.irls_cap()
    R, info = IRLS_GM_batch([irls_problem("small"), (Ind, Rij)], return_info=True)[1]
    ref, ref1, tr = cases._once("irls_oracle", lambda: irls_oracle(Rij, Ind, "GM"))
    assert (tr["l1_iters"], tr["irls_iters"], tr["steps"]) == (10, 23, 60)                # tests/test_batch_caps_host.py; about 7 s of CPU
    assert info["l1_iters"] == tr["l1_iters"] and info["irls_iters"] == tr["irls_iters"]
    assert (info["pd_steps"], info["pd_ill"], info["pd_stuck"]) == (tr["steps"], tr["ill"], tr["stuck"])
    assert info["comp_nodes"] == tr["comp_nodes"] and info["comp_edges"] == tr["comp_edges"] and info["warned_edges"] == tr["warned"]
    assert info["cg_unconverged"] == 0
    d1, d = float(np.abs(info["R_l1"] - ref1).max()), float(np.abs(R - ref).max())
    print(f"oracle parity at n = {R.shape[2]}: |R_l1 - ref| = {d1:.3e}, |R - ref| = {d:.3e}")
    assert d1 <= 1e-9, d1
    assert d <= 1e-7, d


# ---- the tree kernel at n = 4096 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True], ids=["as-given", "reversed"])
def test_mst_at_the_cap(lib, reverse):
    """tree_edges against Kruskal, R bit for bit MST()'s and within 1e-12 of propagate (the bound tests/test_gpu_graph_shapes.py:
    _mst_case holds the single call to on a 4096-node path)."""
    from desc_amd import MST, MST_batch
    small = cemp_batch_cases.model("U12")
    items = [("small", small, np.linspace(0.0, 1.0, small.Ind.shape[0]))] + cases.mst_cap()
    items = items[::-1] if reverse else items
    assert max(int(mo.Ind.max()) for _, mo, _ in items) == lib.mst_batch_max_n()
    out = MST_batch([mo for _, mo, _ in items], [S for _, _, S in items], return_info=True)
    for (name, mo, S), (R, info) in zip(items, out):
        tree, (R1, info1) = cases._once(("mst_ref", name), lambda: (kruskal(mo.Ind, S), MST(mo.Ind, mo.RijMat, S, return_info=True)))
        assert np.array_equal(info["tree_edges"], tree), name
        assert np.array_equal(R, R1) and np.array_equal(info["tree_edges"], info1["tree_edges"]), name
        d = float(np.abs(R - cases._once(("mst_prop", name), lambda: propagate(mo.Ind, mo.RijMat, tree))).max())
        print(name, R.shape[2], d)
        assert d < 1e-12, (name, d)


def test_cemp_mst_batch_at_the_cap(lib):
    """The composition on the random 4096-node graph: MST_batch on CEMP_MST_batch's own SVec."""
    from desc_amd import CEMP_MST_batch, MST_batch
    mo = cases.mst_cap()[-1][1]
    R, S, info = CEMP_MST_batch([mo], cemp_batch_cases.params(), return_info=True)[0]
    R1, info1 = MST_batch([mo], [S], return_info=True)[0]
    assert np.array_equal(R, R1) and np.array_equal(info["mst"]["tree_edges"], info1["tree_edges"])
    assert np.array_equal(info1["tree_edges"], kruskal(mo.Ind, S))


# ---- a CSR row of 4096 entries ---------------------------------------------------------------------------------------------------
def gs_degrees(mo):
    from tests.graph_shapes import degrees
    return degrees(mo.Ind)


def cemp_single(hub_id, nsample):
    from desc_amd import CEMP
    mo = cases.row_cap(hub_id)
    return cases._once(("cemp_single", hub_id, nsample), lambda: CEMP(mo.Ind, mo.RijMat, cemp_batch_cases.params(nsample=nsample)))


def cemp_reference(hub_id, nsample):
    from oracle.cemp_oracle import cemp_oracle_batched
    mo = cases.row_cap(hub_id)
    return cases._once(("cemp_ref", hub_id, nsample), lambda: cemp_oracle_batched(mo.Ind, mo.RijMat, 6, cemp_batch_cases.BETA, nsample, 1))


@pytest.mark.parametrize("order", [("small", 2000), (2000, "small"), ("small", 1), ("small", -1)], ids=lambda o: "-".join(map(str, o)))
def test_cemp_at_the_longest_row(lib, order):
    """SVec bit for bit CEMP()'s and within 1e-12 of cemp_oracle_batched (tests/test_gpu_cemp_batch.py); hub -1 is the last node."""
    from desc_amd import CEMP, CEMP_batch
    small = cemp_batch_cases.model("U12")
    hub_id =[k for k in order if k != "small"][0]
    mo = cases.row_cap(hub_id)
    assert int(gs_degrees(mo).max()) == lib.cemp_batch_max_degree()
    got = dict(zip(order, CEMP_batch([small if k == "small" else mo for k in order], cemp_batch_cases.params())))
    assert np.array_equal(got["small"], cases._once("cemp_single_small", lambda: CEMP(small.Ind, small.RijMat, cemp_batch_cases.params())))
    S = got[hub_id]
    err = float(np.abs(S - cemp_reference(hub_id, 50)).max())
    print(order, S.shape[0], "equal to CEMP():", np.array_equal(S, cemp_single(hub_id, 50)), "max |S - oracle|:", err)
    assert np.array_equal(S, cemp_single(hub_id, 50))
    assert err < 1e-12, err


@pytest.mark.parametrize("nsample", [1, 64, 65, 257])
def test_cemp_at_the_longest_row_in_every_sample_count_class(lib, nsample):
    """nsample = 1 and one value of each class of tests/test_gpu_cemp_batch.py::test_nsample_classes (up to 64, up to 256, above)."""
    from desc_amd import CEMP_batch
    mo = cases.row_cap(2000)
    S = CEMP_batch([cemp_batch_cases.model("U12"), mo], cemp_batch_cases.params(nsample=nsample))[1]
    err = float(np.abs(S - cemp_reference(2000, nsample)).max())
    print(nsample, err)
    assert np.array_equal(S, cemp_single(2000, nsample))
    assert err < 1e-12, err


@pytest.mark.parametrize("hub_id", [2000, 1, -1])
def test_samples_of_the_longest_row_are_the_oracle_s(lib, hub_id):
    """desc_cemp_batch_get_samples: the two other edges of every sampled triangle of the hub's 4096 edges, and of 500 other edges, are
    those of the keyed rule (tests/mpls_oracle.py: cemp_stage)."""
    mo = cases.row_cap(hub_id)
    hub = int(np.argmax(gs_degrees(mo))) + 1
    rows = np.union1d(cases.hub_edges(mo, hub), np.arange(0, mo.Ind.shape[0], 50))
    h = lib.CempBatch([arrays(lib, cemp_batch_cases.model("U12")), arrays(lib, mo)], 50, seed=1)
    try:
        smp = h.samples()[1]
    finally:
        h.destroy()
    e_jk, e_ki = cases.sampled_edges_oracle(mo.Ind, rows, 50, 1)
    assert cases.hub_edges(mo, hub).size == lib.cemp_batch_max_degree()
    assert np.array_equal(smp["has_cycle"][rows], e_jk[:, 0] >= 0)
    assert np.array_equal(smp["e_jk"][rows], e_jk) and np.array_equal(smp["e_ki"][rows], e_ki)


def test_lp_batch_at_the_longest_row(lib):
    """The LP alone (rotations=False: the eigen-solve's cap is 278 nodes) on [small, row_cap] against the single path on the same
    problem, as tests/test_gpu_lp_batch.py compares them: array_equal on S, y, k and pos_edges, == on the record."""
    from desc_amd import linprog_sij_batch
    from tests import lp_cases
    from tests.test_gpu_lp_batch import RECORD
    mos = [lp_cases.model("n30"), cases.row_cap(2000)]
    prm = dict(seed=lp_cases.SEED, max_iter=200, return_dual=True)
    outs = linprog_sij_batch(mos, prm, rotations=False, return_info=True)
    p = lib.default_lp_params()
    p.seed = lp_cases.SEED; p.max_iter = 200
    for b, (mo, (S, info)) in enumerate(zip(mos, outs)):
        S1, y1, k1, info1 = lib.lp_sij_run(arrays(lib, mo), p, want_y=True, want_k=True)
        print(b, {key: info["lp"][key] for key in RECORD})
        assert np.array_equal(S, S1) and np.array_equal(info["y"], y1) and np.array_equal(info["k"], k1), b
        assert np.array_equal(info["pos_edges"], info1["pos_edges"]), b
        for key in RECORD:
            assert info["lp"][key] == info1[key], (b, key, info["lp"][key], info1[key])
        assert info["lp"]["iters"] > 0 and info["lp"]["m_pos"] > 0


# ---- the batched PGD with full lane groups ---------------------------------------------------------------------------------------
PGD_NAMES = ("dense", "mid", "sparse")


def pgd_problem(name):
    return dict(dense=cases.pgd_dense, mid=cases.pgd_mid, sparse=cases.pgd_sparse)[name]()


def pgd_params(T, iters, **kw):
    p = c_params(iters, seed=cases.PGD_SEED, **kw)
    p.n_sample_min = T
    return p


def full_group_problem(T):
    """The problem whose longest segment is exactly T (tests/batch_cap_cases.py)."""
    return "mid" if T < cases.PGD_DENSE_MIN_T else "dense"


@pytest.mark.parametrize("T", cases.PGD_T)
def test_pgd_batch_with_full_lane_groups(lib, oracle, T):
    """40 iterations at a constant step 0.01 against the oracle with tests/test_gpu_batch.py: check (structure bit-exact, S0 1e-14, S_vec
    and w 1e-10, objective rtol 1e-12, equal iters_run)."""
    from tests.test_gpu_batch import check, run_batch
    sts, s0, outs = run_batch(lib, [pgd_problem(k) for k in PGD_NAMES], pgd_params(T, 40, lr=0.01), structures=True)
    for k, got_st, got_s0, out in zip(PGD_NAMES, sts, s0, outs):
        st, S0, ref, _, _ = cases.pgd_reference(oracle, k, T, 40, lr=0.01)
        assert_structure_equal(got_st, st)
        assert out["n_sample"] == st["n_sample"]
        check(out, ref, got_s0, S0)
        assert out["iters_run"] == 40
    k = PGD_NAMES.index(full_group_problem(T))
    seg = np.diff(sts[k]["cum_ind"])
    assert outs[k]["n_sample"] == T and int(seg.max()) == T, (T, outs[k]["n_sample"], int(seg.max()))
    if T == 64:
        assert int((seg == 64).sum()) >= 3000


@pytest.mark.parametrize("T", [16, 64])
def test_pgd_batch_step_rules_with_full_lane_groups(lib, oracle, T):
    """The HybridGradient (Adam) set of tests/test_gpu_batch.py: STEP_RULES at its 1e-9, and the lr = 1 early stop (equal stop
    iteration)."""
    from tests.test_gpu_batch import STEP_RULES, check, run_batch
    probs = [pgd_problem(k) for k in PGD_NAMES]
    kw = STEP_RULES["hybrid_adam"]
    refs = [cases.pgd_reference(oracle, k, T, 40, adam=True, **kw) for k in PGD_NAMES]
    mc = sum(st["m_cycle"] for st, *_ in refs)
    adam = (np.zeros(mc), np.zeros(mc))
    _, s0, outs = run_batch(lib, probs, pgd_params(T, 40, **kw), adam=adam)
    for (st, S0, ref, am, av), out, got_s0 in zip(refs, outs, s0):
        check(out, ref, got_s0, S0, tol=1e-9)
        assert np.abs(out["adam_m"] - am).max() <= 1e-9 and np.abs(out["adam_v"] - av).max() <= 1e-9 and np.abs(av).max() > 0
    stop = dict(lr=1.0, patience=5, stop_tol=1e-3)
    refs = [cases.pgd_reference(oracle, k, T, 400, **stop) for k in PGD_NAMES]
    _, s0, outs = run_batch(lib, probs, pgd_params(T, 400, **stop))
    for k, (st, S0, ref, _, _), out, got_s0 in zip(PGD_NAMES, refs, outs, s0):
        print(T, k, out["iters_run"], ref["iters_run"])
        check(out, ref, got_s0, S0)
        assert out["t_end"] == ref["iters_run"]
    assert refs[PGD_NAMES.index(full_group_problem(T))][2]["iters_run"] < 400          # it does stop early


def test_pgd_full_64_lane_groups_do_not_depend_on_the_batch(lib):
    """pgd_dense at T = 64 alone, first and last in the batch: the same bits."""
    from tests.test_gpu_batch import _same_bits, run_batch
    p = pgd_params(64, 40, lr=0.01)
    dense, sparse = pgd_problem("dense"), pgd_problem("sparse")
    _, _, alone = run_batch(lib, [dense], p)
    _, _, first = run_batch(lib, [dense, sparse], p)
    _, _, last = run_batch(lib, [sparse, dense], p)
    assert alone[0]["n_sample"] == 64
    _same_bits(alone[0], first[0])
    _same_bits(alone[0], last[1])

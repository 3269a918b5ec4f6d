"""GPU tests of the batched LP (desc_amd/csrc/lp_batch.hip, _lib.LpBatch, linprog_sij_batch).

The oracle for equality is the single path: _lib.lp_sij_run on the same problem with seed lp_cases.SEED and the same parameters.  Equality
is np.array_equal on S, y, k and pos_edges and == on iters, restarts, converged, viol, pobj and dobj.  Where a batch entry is an entry of
lp_cases.TRAJECTORIES or an lp_cases.plain run it is also compared with that restatement at the tolerances of
tests/test_gpu_lp_kernels.py: 1e-12 on x and y, 1e-9 relative + 1e-15 on the record, equal counts.  A single run is computed once per
(graph, nsample, parameters) and shared by the tests."""
import numpy as np
import pytest

from desc_amd import DESC_refine_batch, _lib, linprog_sij, linprog_sij_batch
from desc_amd.algorithms import _marshal_problems, marshal_edges
from desc_amd.models import Uniform_Topology
from oracle.spectral_oracle import rotation_alignment
from tests import lp_cases as LC
from tests import lp_oracle as O

pytestmark = pytest.mark.gpu

XY_TOL = 1e-12
_single = {}

# (check_every, max_iter, tol, restart)
PRM_A, PRM_B, PRM_C, PRM_D = (64, 1000, 1e-5, 1), (7, 200, 1e-5, 1), (64, 2000, 1e-3, 0), (64, 100, 1e-5, 1)
# (graph, nsample (None: the rule), trajectory of lp_cases it coincides with under the batch's parameters)
BATCH_A = [("n30", None, "n30"), ("book33", 32, "book33_32"), ("book40", 65, "book40_65"), ("hub60", None, "hub60"), ("sparse", None, None),
           ("star12", None, None)]
BATCH_B = [("n30_s5", 33, "n30_33"), ("sparse", 7, None), ("n30", None, None)]
BATCH_C = [("sparse", None, "sparse_norestart"), ("n30", None, None)]
BATCH_D = [("n30", None, "n30_cap100"), ("sparse", None, None)]


def lp_params(prm):
    check_every, max_iter, tol, restart = prm
    p = _lib.default_lp_params()
    p.seed = LC.SEED; p.check_every = check_every; p.max_iter = max_iter; p.tol = tol; p.restart = restart
    return p


def arrays_of(graph):
    mo = LC.model(graph)
    n, ii, jj, rij, _ = marshal_edges(mo.Ind, mo.RijMat)
    return _lib.ProblemArrays(n, ii, jj, rij)


def single(graph, nsample, prm):
    """desc_lp_sij_run_dev on one of lp_cases.GRAPHS -> dict(S, y, k, pos, info), computed once."""
    key = (graph, nsample, prm)
    if key not in _single:
        dp = _lib.DeviceProblem(arrays_of(graph))
        try:
            p = lp_params(prm)
            p.nsample = 0 if nsample is None else nsample
            S, y, k, info = _lib.lp_sij_run(dp, p, want_y=True, want_k=True)
        finally:
            dp.free()
        _single[key] = dict(S=S, y=y, k=k, pos=info["pos_edges"], info=info)
    return _single[key]


def make_handle(entries):
    return _lib.LpBatch([arrays_of(g) for g, *_ in entries], [ns for _, ns, *_ in entries], seeds=[LC.SEED] * len(entries))


def run_batch(entries, prm, handle=None):
    """-> per entry dict(S, y, k, pos, info) of one batched run (a fresh handle unless one is given)."""
    h = handle if handle is not None else make_handle(entries)
    try:
        outs, _ = h.run(lp_params(prm), want_y=True)
        smp = h.samples()
    finally:
        if handle is None:
            h.destroy()
    return [dict(S=S, y=y, k=s["k"], pos=s["pos_edges"], info=info) for (S, y, info), s in zip(outs, smp)]


RECORD = ("nsample", "m_pos", "rows", "iters", "restarts", "converged", "viol", "pobj", "dobj")


def assert_same(got, ref, label=""):
    """Bit for bit: everything one run returns for a problem against another run's."""
    for key in ("S", "y", "k", "pos"):
        assert np.array_equal(got[key], ref[key]), (label, key)
    for key in RECORD:
        assert got["info"][key] == ref["info"][key], (label, key, got["info"][key], ref["info"][key])


def assert_follows(label, got, ref, graph, nsample):
    """A run against a pdhg_loop result of lp_cases, as tests/test_gpu_lp_kernels.py compares the single path."""
    own, va, vb, d, pos, k_ref, ns = LC.arrays(graph, nsample)
    info = got["info"]
    assert info["nsample"] == ns and info["m_pos"] == pos.size and info["rows"] == 2 * pos.size * ns
    assert np.array_equal(got["pos"], pos) and np.array_equal(got["k"], k_ref)
    off = np.ones(got["S"].size, dtype=bool); off[pos] = False
    assert np.all(got["S"][off] == 1.0)
    dx = float(np.abs(got["S"][pos] - ref["x"]).max()); dy = float(np.abs(got["y"] - ref["y"]).max())
    rec = [(info[key], float(r)) for key, r in zip(("viol", "pobj", "dobj"), ref["rec"])]
    print("%s: iters %d restarts %d converged %d  max|x - x_ref| %.3e  max|y - y_ref| %.3e  viol %.3e (off by %.1e)  P %.12g (%.1e)  D %.12g (%.1e)"
          % ((label, info["iters"], info["restarts"], info["converged"], dx, dy) + tuple(v for g, r in rec for v in (g, abs(g - r)))))
    assert (info["iters"], info["restarts"], info["converged"]) == (ref["iters"], ref["restarts"], int(ref["converged"]))
    assert dx <= XY_TOL and dy <= XY_TOL
    for g, r in rec:
        assert abs(g - r) <= 1e-9 * abs(r) + 1e-15, (g, r)


def assert_empty_lp(got, graph):
    assert np.array_equal(got["S"], np.ones(LC.model(graph).Ind.shape[0]))
    info = got["info"]
    assert info["m_pos"] == info["rows"] == info["iters"] == 0 and info["converged"] == 1
    assert got["y"].size == 0 and got["k"].size == 0 and got["pos"].size == 0


@pytest.mark.parametrize("name,entries,prm", [("A", BATCH_A, PRM_A), ("B", BATCH_B, PRM_B), ("C", BATCH_C, PRM_C), ("D", BATCH_D, PRM_D)])
def test_mixed_batch_equals_the_single_path(name, entries, prm):
    """A: 32 and 64 lanes, a second pass of a lane through t += G (65 samples), a list of 5200 in k_lp_sort's global-memory branch, edges
    without a cycle and an empty LP in the middle.  B: checks every 7 steps, restarts of both kinds close together.  C: checks without
    averages and the stop they lead to.  D: the stop at max_iter off the check grid."""
    outs = run_batch(entries, prm)
    for got, (graph, nsample, traj) in zip(outs, entries):
        label = "batch %s %s/%s" % (name, graph, nsample)
        if graph == "star12":
            assert_empty_lp(got, graph)
        assert_same(got, single(graph, nsample, prm), label)
        if traj is not None:
            assert LC.TRAJECTORIES[traj] == (graph, nsample) + prm
            assert_follows(label, got, LC.trajectory(traj), graph, nsample)
    if name == "A":
        assert LC.longest_list("book40", 65) == 5200 > 2048
    iters = [o["info"]["iters"] for o in outs]
    print("batch %s: iters %s restarts %s converged %s" % (name, iters, [o["info"]["restarts"] for o in outs], [o["info"]["converged"] for o in outs]))


def test_no_step_returns_the_start_and_its_record():
    """max_iter = 0: x = 0, y = 0 and the record of that point (viol = max d, P = D = 0), with the samples."""
    entries, prm = [("n30", None), ("sparse", 7)], (64, 0, 1e-4, 1)
    for got, (graph, nsample) in zip(run_batch(entries, prm), entries):
        assert_same(got, single(graph, nsample, prm), graph)
        assert_follows("%s max_iter 0" % graph, got, LC.loop(graph, nsample, 0, 1e-4), graph, nsample)
        assert np.all(got["S"][got["pos"]] == 0.0) and np.all(got["y"] == 0.0)
        info = got["info"]
        assert info["converged"] == 0 and info["iters"] == 0 and info["pobj"] == 0.0 and info["dobj"] == 0.0 and info["viol"] > 0.0


def test_lane_classes_in_one_batch():
    """18 problems, n30 and sparse with every nsample of lp_cases.LANE_NSAMPLES: the 32- and the 64-lane branch of the row kernels side
    by side in one launch, a second and third cycle per lane above 64.  One handle, 2 and 50 plain steps."""
    entries = [(g, ns) for g in ("n30", "sparse") for ns in LC.LANE_NSAMPLES]
    h = make_handle(entries)
    try:
        for N in (2, 50):
            prm = (64, N, 0.0, 0)
            for got, (graph, nsample) in zip(run_batch(entries, prm, h), entries):
                label = "%s nsample %d N %d" % (graph, nsample, N)
                assert_same(got, single(graph, nsample, prm), label)
                assert_follows(label, got, LC.plain(graph, nsample, N), graph, nsample)
    finally:
        h.destroy()


def test_virtual_grids_beyond_one_pass():
    """m_pos above 32768 (U370) and above 16384 with 64 lanes (U270): the problems' own grids sit at their caps of 2048 and 4096 blocks
    and every workgroup makes a second pass with the stride of its problem's grid, next to a small problem in the same launch."""
    entries, prm = [("n30", None), ("U370", 8), ("U270", 40)], (64, 3, 0.0, 0)
    h = make_handle(entries)
    try:
        assert h.m_pos[1] > 32768 and h.m_pos[2] > 16384
        for got, (graph, nsample) in zip(run_batch(entries, prm, h), entries):
            assert_same(got, single(graph, nsample, prm), graph)
            assert_follows("%s N 3" % graph, got, LC.plain(graph, nsample, 3), graph, nsample)
    finally:
        h.destroy()


def test_scan_chunks_of_the_batched_incidence():
    """k_lpb_scan: a workgroup per problem with k_lp_scan's chunks -- the last thread idle at 1023 variables, every thread busy at 1024,
    chunks of 2 at 1025, of 3 at 2049 -- each starting at its problem's offset in the batch's lists."""
    entries, prm = [("band%d" % mp, 4) for mp in (1023, 1024, 1025, 2049)], (64, 3, 0.0, 0)
    outs = run_batch(entries, prm)
    for got, (graph, nsample), mp in zip(outs, entries, (1023, 1024, 1025, 2049)):
        assert got["info"]["m_pos"] == mp
        assert_same(got, single(graph, nsample, prm), graph)
        assert_follows("%s N 3" % graph, got, LC.plain(graph, nsample, 3), graph, nsample)


def test_stopped_problems_are_frozen():
    """Three problems that converge at different steps (tests/test_gpu_lp_kernels.py: 1792, 2688 and 4480): the first two stay exactly
    what they were at their stop while the third runs on."""
    entries, prm = [("book32", 32), ("book33", 32), ("book40", 65)], (64, 20000, 1e-4, 1)
    refs = [single(g, ns, prm) for g, ns in entries]
    stops = [r["info"]["iters"] for r in refs]
    print("single stops:", stops)
    assert len(set(stops)) == 3
    for got, ref, (graph, _) in zip(run_batch(entries, prm), refs, entries):
        assert_same(got, ref, graph)
        assert got["info"]["converged"] == 1


def test_result_does_not_depend_on_the_batch():
    """Batch A as given, reversed, with one problem twice, and every problem alone: the same bits each time."""
    base = [(g, ns) for g, ns, _ in BATCH_A]
    ref = run_batch(base, PRM_A)
    for got, want in zip(run_batch(base[::-1], PRM_A), ref[::-1]):
        assert_same(got, want, "reversed")
    dup = base[:2] + [base[1]] + base[2:]
    outs = run_batch(dup, PRM_A)
    for got, want in zip(outs, ref[:2] + [ref[1]] + ref[2:]):
        assert_same(got, want, "duplicated")
    for e, want in zip(base, ref):
        assert_same(run_batch([e], PRM_A)[0], want, "alone %s" % e[0])


def test_handle_runs_again_with_other_parameters():
    base_a = [(g, ns) for g, ns, _ in BATCH_A]
    h, other = make_handle(base_a), make_handle(BATCH_D)          # two handles alive at once
    try:
        first = run_batch(base_a, PRM_A, h)
        mid = run_batch(base_a, PRM_D, h)
        third = run_batch(base_a, PRM_A, h)
        d = run_batch(BATCH_D, PRM_D, other)
    finally:
        h.destroy(); other.destroy()
    fresh = run_batch(base_a, PRM_A)
    for a, b, c in zip(first, third, fresh):
        assert_same(a, b, "first against third")
        assert_same(a, c, "against a fresh handle")
    for got, (g, ns) in zip(mid, base_a):
        if g != "star12":
            assert got["info"]["iters"] == 100
        assert_same(got, single(g, ns, PRM_D), "run with D's parameters %s" % g)
    for got, (g, ns, _) in zip(d, BATCH_D):
        assert_same(got, single(g, ns, PRM_D), "second handle %s" % g)


# ---- the whole call
def _graphs():
    from tests.test_gpu_lp import GRAPHS
    return [GRAPHS[name]() for name in ("n30-q0.3", "n60-q0.2", "nonuniform70", "sparse")]


def test_whole_call_against_linprog_sij_and_the_batched_stages():
    """linprog_sij_batch with default parameters and seed 3: S_vec bit for bit linprog_sij's; R_gcw and R_est against the dense
    restatement lp_oracle.tail at tests/test_gpu_lp.py's 1e-8 and 1e-7 after alignment (on the three connected graphs that file compares:
    the sparse graph of 60 nodes is not connected, its rotations are defined per component only); R_est and R_gcw bit for bit the
    batched refinement's and the batched eigen-solve's on the same inputs."""
    models = _graphs()
    problems = [(mo.Ind, mo.RijMat) for mo in models]
    outs = linprog_sij_batch(problems, dict(seed=3, return_dual=True), return_info=True)
    assert len(outs) == 4
    for b, ((R_est, S_vec, info), mo) in enumerate(zip(outs, models)):
        R1, S1, info1 = linprog_sij(mo.Ind, mo.RijMat, dict(seed=3, return_dual=True), return_info=True)
        assert np.array_equal(S_vec, S1) and np.array_equal(info["y"], info1["y"]) and np.array_equal(info["k"], info1["k"])
        assert np.array_equal(info["pos_edges"], info1["pos_edges"])
        for key in RECORD:
            assert info["lp"][key] == info1["lp"][key], (b, key)
        assert info["lp"]["converged"] == 1
        if b < 3:
            R_gcw_ref, R_est_ref = O.tail(mo.Ind, mo.RijMat, S_vec)
            d_gcw = np.abs(rotation_alignment(info["R_gcw"], R_gcw_ref)[0] - R_gcw_ref).max()
            d_est = np.abs(rotation_alignment(R_est, R_est_ref)[0] - R_est_ref).max()
            print("problem %d: iters %d  aligned max|R_gcw - ref| %.3e  max|R_est - ref| %.3e  refine iters %d" % (b, info["lp"]["iters"], d_gcw, d_est, info["refine"]["iters"]))
            assert info["refine"]["cg_unconverged"] == 0 and info["spectral"]["converged"]
            assert d_gcw < 1e-8 and d_est < 1e-7
    S_list, G_list = [o[1] for o in outs], [o[2]["R_gcw"] for o in outs]
    for R, (R_est, _, _) in zip(DESC_refine_batch(problems, S_list, G_list, 1e-3, 200), outs):
        assert np.array_equal(R, R_est)
    probs, perms = _marshal_problems(problems)
    assert all(perm is None for perm in perms)
    gb = _lib.GcwBatch(probs)
    try:
        gcw, _ = gb.run(weights=np.exp(-5.0 * np.concatenate(S_list)), normalize_rows=True)
    finally:
        gb.destroy()
    for (R, _), G in zip(gcw, G_list):
        assert np.array_equal(R, G)
    plain = linprog_sij_batch(problems, dict(seed=3))
    for (R, S), (R_est, S_vec, _) in zip(plain, outs):
        assert np.array_equal(R, R_est) and np.array_equal(S, S_vec)


def test_lp_alone_takes_what_the_eigen_solve_refuses_and_rows_may_be_permuted():
    models = _graphs()
    big = Uniform_Topology(300, 0.05, 0.2, 0.05, "uniform", seed=7)
    assert big.Ind.max() > _lib.gcw_batch_max_n()
    prm = dict(seed=3, max_iter=200)
    with pytest.raises(ValueError, match="solve it with linprog_sij"):
        linprog_sij_batch([models[0], big], prm)
    perm = np.random.default_rng(0).permutation(models[1].Ind.shape[0])
    permuted = (models[1].Ind[perm], models[1].RijMat[:, :, perm])
    S = linprog_sij_batch([models[0], big, models[1], permuted], prm, rotations=False)
    assert len(S) == 4 and S[1].shape == (big.Ind.shape[0],)
    assert np.array_equal(S[3], S[2][perm])
    with_info = linprog_sij_batch([models[1], permuted], prm, rotations=False, return_info=True)
    assert np.array_equal(with_info[0][0], S[2]) and np.array_equal(with_info[1][0], S[3])
    assert np.array_equal(perm[with_info[1][1]["pos_edges"]], with_info[0][1]["pos_edges"])      # the same variables, as rows of either Ind
    n, ii, jj, rij, _ = marshal_edges(big.Ind, big.RijMat)
    p = _lib.default_lp_params()
    p.seed = 3; p.max_iter = 200
    S1, _, _, info1 = _lib.lp_sij_run(_lib.ProblemArrays(n, ii, jj, rij), p, want_k=False)
    assert np.array_equal(S[1], S1) and 0 < info1["m_pos"] < big.Ind.shape[0]

"""GPU tests of the LP solver's kernels (desc_amd/csrc/lp.hip) at their lane, list and restart edges: _lib.lp_sij_run on a DeviceProblem
against tests/lp_oracle.py's pdhg_loop in extended precision, on the cases of tests/lp_cases.py (qualified on the CPU by
tests/test_lp_host.py: no decision of a trajectory case hangs on the last places of a double).

Tolerances: 1e-12 on x and y, the bound of tests/test_gpu_lp.py for the plain recurrence (one ulp of S0Mat moves the cases by at most
8.2e-14); 1e-9 relative + 1e-15 on viol, pobj and dobj, as in test_certificates.  Every test prints what it measured; the docstrings
give the largest figures seen on an MI355X.

Mutation check (a scratch build, never committed): without the swap of d_z / d_zt and d_own / d_ownt after a restart from the average, the
seven trajectory cases that restart from an average fail here, while all of tests/test_gpu_lp.py still passes."""
import numpy as np
import pytest

from desc_amd import _lib
from desc_amd.algorithms import marshal_edges
from tests import lp_cases as LC

pytestmark = pytest.mark.gpu

XY_TOL = 1e-12


def device_run(graph, nsample=None, max_iter=1, tol=0.0, check_every=64, restart=0, perm=None):
    """-> (S (m, sorted edge order), y (m_pos, nsample, 2), k, info) of desc_lp_sij_run_dev on one of lp_cases.GRAPHS."""
    mo = LC.model(graph)
    Ind, Rij = (mo.Ind, mo.RijMat) if perm is None else (mo.Ind[perm], mo.RijMat[:, :, perm])
    n, ii, jj, rij, _ = marshal_edges(Ind, Rij)
    dp = _lib.DeviceProblem(_lib.ProblemArrays(n, ii, jj, rij))
    try:
        p = _lib.default_lp_params()
        p.seed = LC.SEED; p.nsample = 0 if nsample is None else nsample
        p.max_iter = max_iter; p.tol = tol; p.check_every = check_every; p.restart = restart
        return _lib.lp_sij_run(dp, p, want_y=True, want_k=True)
    finally:
        dp.free()


def compare(label, got, ref, graph, nsample):
    """Everything desc_lp_sij_run_dev returns against a pdhg_loop result; -> (max|x - x_ref|, max|y - y_ref|)."""
    S, y, k, info = got
    own, va, vb, d, pos, k_ref, ns = LC.arrays(graph, nsample)
    assert info["nsample"] == ns and info["m_pos"] == pos.size and info["rows"] == 2 * pos.size * ns
    assert np.array_equal(info["pos_edges"], pos) and np.array_equal(k, k_ref)
    off = np.ones(S.size, dtype=bool); off[pos] = False
    assert np.all(S[off] == 1.0)
    dx = float(np.abs(S[pos] - ref["x"]).max()); dy = float(np.abs(y - ref["y"]).max())
    rec = [(info[key], float(r)) for key, r in zip(("viol", "pobj", "dobj"), ref["rec"])]
    print("%s: iters %d restarts %d converged %d  max|x - x_ref| %.3e  max|y - y_ref| %.3e  viol %.3e (off by %.1e)  P %.12g (%.1e)  D %.12g (%.1e)"
          % ((label, info["iters"], info["restarts"], info["converged"], dx, dy) + tuple(v for g, r in rec for v in (g, abs(g - r)))))
    assert (info["iters"], info["restarts"], info["converged"]) == (ref["iters"], ref["restarts"], int(ref["converged"]))
    assert dx <= XY_TOL and dy <= XY_TOL
    for g, r in rec:
        assert abs(g - r) <= 1e-9 * abs(r) + 1e-15, (g, r)
    return dx, dy


@pytest.mark.parametrize("name", list(LC.TRAJECTORIES))
def test_restarted_loop_follows_the_restatement(name):
    """The restarted path step for step: the running sums of k_lp_col<true> / k_lp_row<*, true>, k_lp_average, k_lp_restart, the swap of
    z / own after a restart from the average, the returned point, the stop off the check_every grid and the checks without averages.
    Measured: x within 2.9e-15, y within 4.3e-13 (hub60; 3.8e-13 n30, 2.0e-13 sparse_rule, below 1e-13 on the book graphs), viol within
    2.6e-16, pobj within 4.8e-16 and dobj within 1.6e-15 relative; every count equal."""
    graph, nsample, check_every, max_iter, tol, restart = LC.TRAJECTORIES[name]
    got = device_run(graph, nsample, max_iter, tol, check_every, restart)
    compare(name, got, LC.trajectory(name), graph, nsample)


@pytest.mark.parametrize("nsample", LC.LANE_NSAMPLES)
@pytest.mark.parametrize("graph", ["n30", "sparse"])
def test_lane_classes_follow_the_plain_recurrence(graph, nsample):
    """k_lp_row / k_lp_eval_row: 32 lanes per edge up to 32 samples, 64 above, a second and third cycle per lane through t += G above 64.
    Two steps are the first with K'y != 0; the record after the last step is the work of k_lp_eval_row<32> / <64> and k_lp_eval_col.
    Measured over the 36 runs: x within 8.9e-15, y within 3.3e-14, viol within 8.9e-16, pobj within 5.8e-16 and dobj within 5.1e-14 relative."""
    for N in (2, 50):
        compare("%s nsample %d N %d" % (graph, nsample, N), device_run(graph, nsample, N), LC.plain(graph, nsample, N), graph, nsample)


@pytest.mark.parametrize("graph,nsample,length", [("book32", 32, 2048), ("book33", 32, 2112), ("book40", 65, 5200)])
def test_long_incidence_lists_sort_in_either_branch(graph, nsample, length):
    """k_lp_sort ranks a list of up to 2048 entries in the LDS and a longer one in global memory; k_lp_fill stores in arrival order, so the
    promise of equal bits on two runs rests on that sort.  Measured after 50 plain steps: x within 1.9e-15, y within 8.7e-15, dobj within
    1.8e-14 relative; the restarted runs stop after 1792, 2688 and 4480 steps (9, 11 and 10 restarts) with equal bits."""
    assert LC.longest_list(graph, nsample) == length
    compare("%s plain 50" % graph, device_run(graph, nsample, 50), LC.plain(graph, nsample, 50), graph, nsample)
    prm = dict(max_iter=20000, tol=1e-4, restart=1)
    S1, y1, k1, i1 = device_run(graph, nsample, **prm)
    S2, y2, k2, i2 = device_run(graph, nsample, **prm)
    assert i1["converged"] == 1 and i1["restarts"] > 0
    assert np.array_equal(S1, S2) and np.array_equal(y1, y2) and (i1["iters"], i1["viol"], i1["pobj"], i1["dobj"]) == (i2["iters"], i2["viol"], i2["pobj"], i2["dobj"])
    perm = np.random.default_rng(0).permutation(S1.size)
    S3, y3, k3, i3 = device_run(graph, nsample, perm=perm, **prm)
    print("%s: iters %d restarts %d, the same bits on three runs" % (graph, i1["iters"], i1["restarts"]))
    assert np.array_equal(S3, S1) and np.array_equal(y3, y1) and np.array_equal(k3, k1) and i3["iters"] == i1["iters"]


@pytest.mark.parametrize("graph,nsample,cap", [("U370", 8, 32768), ("U270", 40, 16384)])
def test_grid_stride_passes(graph, nsample, cap):
    """More variables than one pass of the grid holds: 2048 blocks of 16 edges in k_lp_col / k_lp_eval_col, 4096 blocks of 8 in k_lp_row<32>
    (U370, 8 samples), 4096 blocks of 4 in k_lp_row<64> (U270, 40 samples).  Measured: x within 8.7e-17, y within 7.6e-16, the record
    within 1.9e-16 relative."""
    assert LC.arrays(graph, nsample)[4].size > cap
    compare("%s nsample %d N 3" % (graph, nsample), device_run(graph, nsample, 3), LC.plain(graph, nsample, 3), graph, nsample)


@pytest.mark.parametrize("graph,mp", [("band1023", 1023), ("band1024", 1024), ("band1025", 1025), ("band2049", 2049)])
def test_scan_chunks(graph, mp):
    """k_lp_scan: one workgroup of 1024 threads, a chunk of ceil(m_pos / 1024) counts per thread -- the last thread idle at 1023, every
    thread busy at 1024, chunks of 2 with half the threads idle at 1025, chunks of 3 at 2049.  A wrong offset moves tau and K'y.
    Measured: x within 2.7e-15, y within 1.4e-14, the record within 2.8e-16 relative."""
    assert LC.arrays(graph, 4)[4].size == mp
    compare("%s N 3" % graph, device_run(graph, 4, 3), LC.plain(graph, 4, 3), graph, 4)


@pytest.mark.parametrize("graph", ["star12", "bipartite8_9"])
def test_graph_without_a_triangle_is_the_empty_lp(graph):
    S, y, k, info = device_run(graph, None, 100, 1e-4, restart=1)
    assert np.array_equal(S, np.ones(LC.model(graph).Ind.shape[0]))
    assert info["m_pos"] == info["rows"] == info["iters"] == 0 and info["converged"] == 1
    assert y.size == 0 and k.size == 0 and info["pos_edges"].size == 0


@pytest.mark.parametrize("graph,nsample", [("n30", None), ("sparse", 7)])
def test_no_step_with_outputs_requested(graph, nsample):
    """max_iter = 0: the start x = 0, y = 0 and its record (viol = max d, P = D = 0), with the samples.  Measured: no difference at all."""
    got = device_run(graph, nsample, 0, 1e-4, restart=1)
    S, y, k, info = got
    ref = LC.loop(graph, nsample, 0, 1e-4)
    compare("%s max_iter 0" % graph, got, ref, graph, nsample)
    pos = LC.arrays(graph, nsample)[4]
    assert np.all(S[pos] == 0.0) and np.all(y == 0.0) and info["converged"] == 0 and info["iters"] == 0
    assert info["pobj"] == 0.0 and info["dobj"] == 0.0 and info["viol"] > 0.0

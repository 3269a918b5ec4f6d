"""linprog_sij (Algorithms/linprog_sij.m) and DESC_init without a GPU: the new ABI, self-checks of the restatement (tests/lp_oracle.py)
against HiGHS through duality -- the LP optimum is not unique, so no vector is compared element by element -- and argument checks."""
import ctypes as C

import numpy as np
import pytest

from desc_amd.models import Uniform_Topology
from tests import graph_shapes as gs
from tests import lp_cases as LC
from tests import lp_oracle as O


def test_lp_abi_symbols_structs_and_defaults(lib):
    L = lib.load()
    for name in ("desc_lp_params_default", "desc_lp_sij_run", "desc_lp_sij_run_dev"):
        assert hasattr(L, name) and name in lib.EXPORTS
    assert C.sizeof(lib.LpParams) == 48 and C.sizeof(lib.LpInfo) == 104          # as include/desc_amd.h states
    p = lib.default_lp_params()
    assert (p.nsample, p.seed, p.tol, p.max_iter, p.check_every, p.restart, p.verbose) == (0, 0, 1e-4, 200000, 64, 1, 0)
    assert not p.pos_out


@pytest.fixture(scope="module", params=[(30, 0.2), (30, 0.3), (60, 0.2), (60, 0.3)], ids=["n30-q0.2", "n30-q0.3", "n60-q0.2", "n60-q0.3"])
def lp(request):
    n, q = request.param
    mo = Uniform_Topology(n, 0.5, q, 0.05, "uniform", seed=3)
    K, b, pos, k, ns = O.build_lp(mo.Ind, mo.RijMat, 3)
    return mo, K, b, pos, k, ns, O.solve_highs(K, b)


def test_oracle_lp_shape(lp):
    mo, K, b, pos, k, ns, _ = lp
    mp = pos.size
    assert ns == 30 and K.shape == (2 * ns * mp, mp) and k.shape == (mp, ns) and b.shape == (2 * ns * mp,)
    assert np.array_equal(np.asarray(abs(K).sum(axis=1)).reshape(-1), np.full(K.shape[0], 3.0))
    assert np.all(b[0::2] == -b[1::2]) and np.all(b[0::2] >= 0)
    i, j = mo.Ind[pos, 0], mo.Ind[pos, 1]
    assert np.all(k != i[:, None]) and np.all(k != j[:, None]) and k.min() >= 1 and k.max() <= mo.Ind.max()


def test_oracle_certificates_close_on_the_highs_optimum(lp):
    _, K, b, _, _, _, (f, x, y) = lp
    assert np.all(y >= 0) and np.all(x >= 0) and np.all(x <= 1)
    viol, P, D = O.certificates(K, b, x, y)
    print("viol %.3e  P %.12g  D %.12g  f* %.12g" % (viol, P, D, f))
    assert viol <= 1e-9
    assert abs(P - D) <= 1e-7 * (1 + f)


def test_oracle_plain_pdhg_stays_inside_the_duality_bounds(lp):
    """Every y >= 0 is dual feasible (D <= f*), and weak duality against HiGHS's dual bounds P from below:
    c'x + y*'(Kx - b) >= min over the box = f*."""
    _, K, b, _, _, _, (f, xs, ys) = lp
    tau, sigma = O.step_sizes(K)
    assert np.all(sigma == 1.0 / 3.0)
    for N in (1, 50, 2000):
        x, y = O.pdhg_plain(K, b, tau, sigma, N)
        assert np.all(y >= 0) and np.all(x >= 0) and np.all(x <= 1)
        viol, P, D = O.certificates(K, b, x, y)
        print("N %d: viol %.3e  P %.9g  D %.9g  f* %.9g" % (N, viol, P, D, f))
        assert D <= f + 1e-9 * (1 + f)
        assert P >= f - ys @ np.maximum(K @ x - b, 0.0) - 1e-9 * (1 + f)
    assert abs(P - f) < 0.05 * f and viol < 0.05          # 2000 steps: on its way (the bounds above hold at any step)


def test_oracle_edges_without_a_cycle_are_no_variables():
    Ind = np.array([[1, 2], [1, 3], [2, 3], [3, 4], [4, 5]])            # a triangle with a tail
    R = np.repeat(np.eye(3)[:, :, None], 5, axis=2)
    K, b, pos, k, ns = O.build_lp(Ind, R, 0, nsample=4)
    assert list(pos) == [0, 1, 2] and K.shape == (24, 3) and np.all(b == 0)
    assert np.array_equal(k, np.array([[3] * 4, [2] * 4, [1] * 4]))
    assert O.rule_nsample([1, 1, 1]) == 30 and O.rule_nsample([200, 210, 220]) == 53 and O.rule_nsample([]) == 30


def test_linprog_sij_and_desc_init_check_their_arguments():
    from desc_amd import DESC_init, linprog_sij
    from desc_amd import ConstantStepSize
    params = dict(iters=5, Gradient=ConstantStepSize(0.01), verbose=False)
    R0 = np.zeros((3, 3, 0))
    for call in (lambda I, R: linprog_sij(I, R), lambda I, R: DESC_init(I, R, params)):
        with pytest.raises(ValueError, match="empty edge list"):
            call(np.zeros((0, 2), dtype=np.int64), R0)
        with pytest.raises(ValueError, match="m x 2"):
            call(np.array([1, 2, 3]), R0)
        with pytest.raises(ValueError, match="3 x 3 x m"):
            call(np.array([[1, 2], [1, 3]]), np.zeros((3, 3, 5)))
        with pytest.raises(ValueError):
            call(np.array([[2, 1]]), np.zeros((3, 3, 1)))               # Ind(:,1) < Ind(:,2)


# ---- pdhg_loop, the restatement of lp.hip's loop, and the cases of tests/lp_cases.py ---------------------------------------------------
def _dist(a, b):
    return float(max(np.abs(a["x"] - b["x"]).max(), np.abs(a["y"] - b["y"]).max()))


def test_pdhg_loop_without_restarts_is_the_plain_recurrence(lp):
    mo, K, b, pos, k, ns, _ = lp
    own, va, vb, d, pos2, k2, ns2 = O.lp_arrays(mo.Ind, mo.RijMat, 3)
    assert np.array_equal(pos, pos2) and np.array_equal(k, k2) and ns == ns2 and np.array_equal(b[0::2], d.reshape(-1))
    tau, sigma = O.step_sizes(K)
    for N in (1, 2, 50):
        r = O.pdhg_loop(own, va, vb, d, pos.size, ns, N, 0.0, restart=False)
        x, y = O.pdhg_plain(K, b, tau, sigma, N)
        dx, dy = np.abs(r["x"] - x).max(), np.abs(r["y"].reshape(-1) - y).max()
        print("N %d: max|x - x_plain| %.3e  max|y - y_plain| %.3e" % (N, dx, dy))
        assert dx <= 1e-13 and dy <= 1e-13
        assert r["iters"] == N and r["restarts"] == 0 and not r["converged"] and r["log"] == []
        viol, P, D = O.certificates(K, b, x, y)
        for got, ref in zip(r["rec"], (viol, P, D)):
            assert abs(got - ref) <= 1e-12 * (1 + abs(ref))


@pytest.mark.parametrize("name", list(LC.TRAJECTORIES))
def test_trajectory_case_hangs_on_no_last_place(name):
    """Conditions (a) to (c) of tests/lp_cases.py.  Measured: smallest margin 6.1e-4 (book40_65, average against iterate at step 1000), then 2.2e-3
    (n30_33) and 2.5e-3 (sparse_7); float64 against extended precision at most 7.6e-15; one ulp of S0Mat moves x, y by at most 8.2e-14 (book33_32)."""
    ext, f64 = LC.trajectory(name), LC.trajectory(name, np.float64)
    worst = min((v, key, g["it"]) for g in ext["log"] for key, v in g["margins"].items())
    d64 = _dist(ext, f64)
    moved = [_dist(ext, LC.trajectory(name, perturb=s)) for s in (1, 2, 3)]
    print("%s: iters %d restarts %d converged %d  smallest margin %.3e (%s at step %d)  |f64 - ext| %.2e  moved by one ulp of S0Mat %s"
          % (name, ext["iters"], ext["restarts"], ext["converged"], worst[0], worst[1], worst[2], d64, " ".join("%.2e" % v for v in moved)))
    assert np.finfo(np.longdouble).eps < 2e-19                                              # the extended run is one
    assert worst[0] >= 1e-4                                                                 # (a)
    assert O.same_decisions(ext, f64) and d64 <= 1e-13                                      # (b)
    for s in (1, 2, 3):                                                                     # (c)
        assert O.same_decisions(ext, LC.trajectory(name, perturb=s))
    assert max(moved) <= 1e-13


@pytest.mark.parametrize("graph,nsample", LC.COMPARED, ids=["%s-%s" % c for c in LC.COMPARED])
def test_s0mat_is_well_conditioned_on_every_compared_graph(graph, nsample):
    """The device evaluates S0Mat itself, so the comparisons at 1e-12 also need an S0Mat that does not hang on the last place of a rotation:
    acos turns one ulp of a trace into 1e-16 / sin(angle).  Under +-1 ulp of RijMat (gs.ulp_perturbed) S0Mat moves by at most 5.2e-14 on these
    graphs (band1024); Uniform_Topology(270, 0.5, 0.2, 0.05, seed=3) at 40 samples, not used for that reason, gives 2.4e-10."""
    mo = LC.model(graph)
    d = LC.arrays(graph, nsample)[3]
    moved = max(float(np.abs(O.lp_arrays(mo.Ind, gs.ulp_perturbed(mo.RijMat, s), LC.SEED, nsample)[3] - d).max()) for s in (1, 2))
    print("%s nsample %s: S0Mat in [%.2e, %.6f], moved %.2e" % (graph, nsample, d.min(), d.max(), moved))
    assert moved <= 1e-13


def test_trajectory_cases_reach_what_they_are_there_for():
    restarted = [name for name, c in LC.TRAJECTORIES.items() if c[5] and c[3] >= 200]
    assert len(restarted) == 7
    for name in restarted:                                                                  # both kinds of restart, in every case
        kinds = {g["avg"] for g in LC.trajectory(name)["log"] if g["fired"]}
        assert kinds == {True, False}, name
    fired = {g["fired"] for name in restarted for g in LC.trajectory(name)["log"]}
    assert fired == {None, "0.2", "0.8+grew", "period"}                                     # every restart condition, and checks without one
    cap = LC.trajectory("n30_cap100")
    assert cap["iters"] == 100 and [g["it"] for g in cap["log"]] == [64, 100] and cap["log"][-1]["fired"] is None and not cap["converged"]
    it7, itr, itn = LC.trajectory("sparse_7"), LC.trajectory("sparse_rule"), LC.trajectory("sparse_norestart")
    assert it7["converged"] and it7["iters"] == 280 and not it7["log"][-1]["avg"]           # stops on the iterate
    assert itr["converged"] and itr["iters"] == 512 and itr["log"][-1]["avg"]               # stops on the average
    assert itn["converged"] and itn["iters"] == 384 and itn["restarts"] == 0 and all("avg" not in g["margins"] for g in itn["log"])
    for name in ("n30", "n30_33", "book33_32", "book40_65", "hub60"):                       # stop at the cap
        r = LC.trajectory(name)
        assert not r["converged"] and r["iters"] == LC.TRAJECTORIES[name][3] and 5 <= r["restarts"] <= 7
    assert LC.model("sparse").Ind.shape[0] > LC.arrays("sparse", 7)[4].size > 0             # edges without a cycle


def test_book_graphs_have_the_list_lengths_of_the_sort_branches():
    """k_lp_sort keeps a list of up to 2048 entries in the LDS: the spine of book(pages) is in 2 pages nsample cycles."""
    for graph, nsample, length in (("book32", 32, 2048), ("book33", 32, 2112), ("book40", 65, 5200)):
        mo = LC.model(graph)
        pages = mo.Ind.shape[0] // 2
        assert mo.Ind.shape[0] == 2 * pages + 1 <= 81 and int(mo.Ind.max()) == pages + 2 <= 42
        codeg = gs.codegrees(mo.Ind)
        assert codeg[0] == pages and np.all(codeg[1:] == 1) and tuple(mo.Ind[0]) == (1, 2)
        own, va, vb, d, pos, k, ns = LC.arrays(graph, nsample)
        inc = np.bincount(va, minlength=pos.size) + np.bincount(vb, minlength=pos.size)
        assert ns == nsample and pos.size == 2 * pages + 1
        assert inc[0] == length == 2 * pages * nsample == LC.longest_list(graph, nsample) and np.all(inc[1:] <= 2 * nsample)
        assert O.rule_nsample(codeg) == 30 and LC.arrays(graph)[6] == 30


def test_scan_and_grid_stride_graphs_have_their_sizes():
    for graph, mp in (("band1023", 1023), ("band1024", 1024), ("band1025", 1025), ("band2049", 2049)):
        mo = LC.model(graph)
        assert mo.Ind.shape[0] == mp and np.all(gs.codegrees(mo.Ind) > 0)
    assert LC.arrays("U370", 8)[4].size == 34081 and LC.arrays("U270", 40)[4].size == 18144
    for graph in ("star12", "bipartite8_9"):
        assert np.all(gs.codegrees(LC.model(graph).Ind) == 0)

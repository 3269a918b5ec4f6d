"""TEST INFRASTRUCTURE -- the problems of the LP kernel tests (tests/test_lp_host.py, tests/test_gpu_lp_kernels.py), built once per process,
and the answers of tests/lp_oracle.py's pdhg_loop, computed once and shared.

A trajectory case is a run of the restarted loop that the device has to follow decision by decision.  That is a fair demand only where
no decision hangs on the last places of a double; tests/test_lp_host.py checks for every case below that
  (a) every comparison pdhg_loop evaluated has a relative margin of at least 1e-4,
  (b) its float64 and extended-precision runs take the same decisions and differ by at most 1e-13,
  (c) with S0Mat moved by one ulp (gs.ulp_perturbed, seeds 1 to 3) the decisions stay and x, y move by at most 1e-13.
A case that fails one of them is replaced by another seed or size of the same family that reaches the same branch, never excused."""
import numpy as np

from desc_amd.models import Uniform_Topology
from tests import graph_shapes as gs
from tests import lp_oracle as O

SEED = 3
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


GRAPHS = {
    "n30": lambda: Uniform_Topology(30, 0.5, 0.2, 0.05, "uniform", seed=3),
    "n30_s5": lambda: Uniform_Topology(30, 0.5, 0.2, 0.05, "uniform", seed=5),
    "sparse": lambda: Uniform_Topology(60, 0.08, 0.2, 0.05, "uniform", seed=5),
    "book32": lambda: gs.book(32, seed=7),
    "book33": lambda: gs.book(33, seed=7),
    "book40": lambda: gs.book(40, seed=7),
    "hub60": lambda: gs.hub(60, 0.1, [30], seed=11),
    # the grid-stride passes: m_pos above 32768 (k_lp_col, k_lp_eval_col, k_lp_row<32>) and above 16384 (k_lp_row<64>).  Noise but no outliers:
    # among the 2.7e5 and 7.3e5 cycles of these graphs with q = 0.2 some Haar outlier cycles turn by pi - 1e-6, where acos makes 2.4e-10 of S0Mat
    # out of one ulp of a rotation (tests/test_lp_host.py measures it; tests/graph_shapes.py: SHAPES says the same of CEMP's graphs)
    "U370": lambda: Uniform_Topology(370, 0.5, 0.0, 0.3, "uniform", seed=3),
    "U270": lambda: Uniform_Topology(270, 0.5, 0.0, 0.3, "uniform", seed=3),
    # k_lp_scan's chunks: band(n, 2) has 2 n - 3 edges, all on a triangle; the chord {1, 4} (common neighbours 2 and 3) makes the count even
    "band1023": lambda: gs.band(513, 2, seed=9),
    "band1024": lambda: gs.band(513, 2, seed=9, chords=[(1, 4)]),
    "band1025": lambda: gs.band(514, 2, seed=9),
    "band2049": lambda: gs.band(1026, 2, seed=9),
    # no triangle at all
    "star12": lambda: gs.star(12, 3, seed=38),
    "bipartite8_9": lambda: gs.bipartite(8, 9, 0.4, seed=14),
}

# name -> (graph, nsample (None: the rule), check_every, max_iter, tol, restart); the branch a case is there for is in its comment.
TRAJECTORIES = {
    # G = 32 lanes at the rule's 30 samples, every edge a variable; 1000 steps: restarts from the average and from the iterate, stop at the cap
    "n30": ("n30", None, 64, 1000, 1e-5, 1),
    # G = 64 with one lane past 32, checks every 7 steps: many checks, restarts of either kind close together.  On graph seed 5: on seed 3 the
    # check at step 175 follows a restart at 112 and compares cnt = 63 with 0.36 * 175 = 63, a margin of 0 (condition (a))
    "n30_33": ("n30_s5", 33, 7, 200, 1e-5, 1),
    # edges without a cycle (k_lp_vars maps edge ids to variables), 7 samples in a 32-lane group; converges on the iterate
    "sparse_7": ("sparse", 7, 7, 300, 1e-5, 1),
    # the same graph at the rule's nsample: converges on the average, which is then the returned point
    "sparse_rule": ("sparse", None, 64, 3000, 1e-5, 1),
    # the spine's incidence list of 2112 entries: k_lp_sort's global-memory branch feeding K'y for 1000 restarted steps
    "book33_32": ("book33", 32, 64, 1000, 1e-5, 1),
    # 65 samples: the second pass of a lane through t += G, in k_lp_row<64, true> and k_lp_eval_row<64>; a list of 5200
    "book40_65": ("book40", 65, 64, 1000, 1e-5, 1),
    # one long incidence row among short ones
    "hub60": ("hub60", None, 64, 1000, 1e-5, 1),
    # the stop at it == max_iter off the check_every grid: the last check is at step 100 = 64 + 36
    "n30_cap100": ("n30", None, 64, 100, 1e-5, 1),
    # restart = 0 with tol > 0: checks of the iterate alone, no averages kept (k_lp_col<false>, k_lp_row<32, false>), and the stop they lead to
    # at step 384.  On the sparse graph: n30 needs 1664 plain steps, over which one ulp of S0Mat moves y by 1.9e-13 (condition (c))
    "sparse_norestart": ("sparse", None, 64, 2000, 1e-3, 0),
}


# (graph, nsample) of every run that tests/test_gpu_lp_kernels.py compares at 1e-12
LANE_NSAMPLES = [1, 7, 31, 32, 33, 63, 64, 65, 129]
COMPARED = sorted({(c[0], c[1]) for c in TRAJECTORIES.values()} | {(g, ns) for g in ("n30", "sparse") for ns in LANE_NSAMPLES}
                  | {("book32", 32), ("book33", 32), ("book40", 65), ("U370", 8), ("U270", 40)} | {("band%d" % mp, 4) for mp in (1023, 1024, 1025, 2049)},
                  key=str)


def model(graph):
    return _once(("model", graph), GRAPHS[graph])


def arrays(graph, nsample=None):
    """lp_oracle.lp_arrays of one of GRAPHS at SEED -> (own, va, vb, d, pos, k, nsample)."""
    return _once(("arrays", graph, nsample), lambda: O.lp_arrays(model(graph).Ind, model(graph).RijMat, SEED, nsample))


def loop(graph, nsample, max_iter, tol, check_every=64, restart=1, dtype=np.longdouble, perturb=None):
    """pdhg_loop on one of GRAPHS, computed once per parameter set.  perturb: the seed of gs.ulp_perturbed applied to S0Mat."""
    def make():
        own, va, vb, d, pos, k, ns = arrays(graph, nsample)
        if perturb is not None:
            d = gs.ulp_perturbed(d, perturb)
        return O.pdhg_loop(own, va, vb, d, pos.size, ns, max_iter, tol, check_every=check_every, restart=bool(restart), dtype=dtype)
    return _once(("loop", graph, nsample, max_iter, tol, check_every, restart, np.dtype(dtype).name, perturb), make)


def trajectory(name, dtype=np.longdouble, perturb=None):
    graph, nsample, check_every, max_iter, tol, restart = TRAJECTORIES[name]
    return loop(graph, nsample, max_iter, tol, check_every, restart, dtype, perturb)


def plain(graph, nsample, N, dtype=np.longdouble):
    """N plain steps (restart = 0, tol = 0) from x = 0, y = 0."""
    return loop(graph, nsample, N, 0.0, 64, 0, dtype)


def longest_list(graph, nsample=None):
    """The longest incidence list: how often one variable is the edge ik or jk of a cycle."""
    own, va, vb, d, pos, k, ns = arrays(graph, nsample)
    return int((np.bincount(va, minlength=pos.size) + np.bincount(vb, minlength=pos.size)).max())

"""TEST INFRASTRUCTURE -- the inputs of the primal-dual solver's tests (tests/test_pd_host.py, tests/test_gpu_pd_kernels.py,
tests/test_gpu_pd_solver.py), built once per process and left unchanged.

A solver case is (graph, seed, scale, pdmaxiter): B = scale * the edge log map at the spanning-tree start of the graph's problem, as
the L1 stage first sees it.  Graphs: "u8" / "u12" / "u16" / "u30" = Uniform_Topology(n, 0.5, 0.1, 0.05, "uniform", seed) (p raised to
0.7 for n = 8 so that the graph is connected at every seed), "k6" = the complete graph on 6 nodes with rotations of the same noise
model.  SEARCH_SPACE is the finite space the exit search of tests/test_pd_host.py's docstring ran over; FOUND records the first case
(in the order of SEARCH_SPACE) that restatement (a) takes through each exit."""
import numpy as np

from tests import irls_oracle as IO
from tests import laa_maps_cases as K
from tests import pd_oracle as P

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


GRAPHS = ("u8", "u12", "u16", "u30", "k6")
SEARCH_SPACE = [(g, seed, scale, 64) for g in GRAPHS for seed in range(10) for scale in (1.0, 1e-3, 1e3)]

# what the search found: name -> (case, step, note).  None: not reached anywhere in SEARCH_SPACE (tests/test_pd_host.py says so).
FOUND = {
    "stuck_while_another_goes_on": dict(case=("u8", 1, 1e-3, 64), coordinate=0, step=19),      # the others take part in step 20
    "cg_breakdown": dict(case=("u8", 0, 1.0, 64), coordinate=0, step=11),                      # B finite; coordinate 2 goes on to step 13
    "tol": None,                                                                               # sdg < eps: by no case of SEARCH_SPACE
    "three_trial_counts": dict(case=("u8", 0, 1e-3, 64), step=13, trials=(28, 1, 4)),
    "cg_cap": dict(case=("u8", 0, 1.0, 64), step=12),                                          # 20 n + 200 = 360 CG steps, unconverged
}
SOLVER_CASES = sorted({v["case"] for v in FOUND.values() if v})


def _sorted_problem(Ind, RijMat):
    Ind = np.asarray(Ind, dtype=np.int64)
    order = np.lexsort((Ind[:, 1], Ind[:, 0]))
    return Ind[order], np.asarray(RijMat)[:, :, order]


def problem(graph, seed):
    """-> (n, ii, jj (0-based, sorted), RijMat (3, 3, m))."""
    def make():
        from desc_amd.models import Uniform_Topology
        if graph == "k6":
            rng = np.random.default_rng(600 + seed)
            n, ii, jj = K.complete_graph(6)
            R = np.linalg.qr(rng.standard_normal((6, 3, 3)))[0]
            R[np.linalg.det(R) < 0, :, 0] *= -1
            Rij = np.empty((3, 3, len(ii)))
            for e, (i, j) in enumerate(zip(ii, jj)):
                if rng.uniform() < 0.1:
                    N = np.linalg.qr(rng.standard_normal((3, 3)))[0]
                else:
                    N = np.linalg.qr(np.eye(3) + 0.05 * rng.standard_normal((3, 3)))[0]
                N = N if np.linalg.det(N) > 0 else -N
                Rij[:, :, e] = R[i] @ R[j].T @ N
            return n, ii.astype(np.int64), jj.astype(np.int64), Rij
        n = int(graph[1:])
        mo = Uniform_Topology(n, 0.7 if n == 8 else 0.5, 0.1, 0.05, "uniform", seed=seed)
        Ind, Rij = _sorted_problem(mo.Ind, mo.RijMat)
        assert int(Ind.max()) == n
        return n, Ind[:, 0] - 1, Ind[:, 1] - 1, Rij
    return _once(("problem", graph, seed), make)


def edge_log_start(graph, seed):
    """B (m, 3) of BoxMedianSO3Graph.m:143-160 at the spanning-tree start (tests/irls_oracle.py), and the problem."""
    def make():
        n, ii, jj, Rij = problem(graph, seed)
        RR, _ = IO.project(np.transpose(Rij, (1, 0, 2)))
        from oracle.refine_oracle import R2Q
        QQ = R2Q(RR)
        I = np.stack([ii + 1, jj + 1])
        Q, _, _ = IO.tree_start(I, QQ, n)
        return n, ii, jj, IO.edge_log(I, Q, QQ)
    return _once(("B", graph, seed), make)


def case_inputs(case):
    graph, seed, scale, pdmaxiter = case
    n, ii, jj, B = edge_log_start(graph, seed)
    return n, ii, jj, B * scale, pdmaxiter


def solved(case, watch_steps=None):
    """Restatement (a) of the case, once per process.  watch_steps: also keep, per (step, stage), the (before, scal, after, part) of the
    first launch of that stage in those steps -> (result, seen)."""
    def make():
        n, ii, jj, B, pdmaxiter = case_inputs(case)
        seen = {}

        def watch(step, stage, before, scal, after, part):
            if watch_steps is not None and step in watch_steps and (step, stage) not in seen:
                seen[(step, stage)] = (P.copy(before), scal, P.copy(after), None if part is None else part.copy())
        return P.solve(n, ii, jj, B, pdmaxiter, watch=watch), seen
    return _once(("solved", case, None if watch_steps is None else tuple(watch_steps)), make)


def lu_reference(case):
    """tests/irls_oracle.py's l1decode_pd (dense LU), coordinate by coordinate -> x (n, 3) with row 0 = 0, and the per-coordinate traces."""
    def make():
        n, ii, jj, B, pdmaxiter = case_inputs(case)
        A = IO.amatrix(np.stack([ii + 1, jj + 1]), n)
        x = np.zeros((n, 3)); traces = []
        for c in range(3):
            tr = {}
            x[1:, c] = IO.l1decode_pd(np.zeros(n - 1), A, B[:, c], IO.EPS, pdmaxiter, trace=tr)
            traces.append(dict(steps=tr.get("steps", 0), ill=tr.get("ill", 0), stuck=tr.get("stuck", 0)))
        return x, traces
    return _once(("lu", case), make)


def describe(res):
    """What a solve did, per coordinate: the steps it took part in, how it ended, and the trial counts."""
    tr = res["trace"]
    out = []
    for c in range(3):
        steps = [k for k in range(1, tr.shape[0]) if tr[k, c, 0]]
        end = "maxiter"
        if steps:
            last = tr[steps[-1], c]
            if last[1]: end = "ill"
            elif last[4] == P.STUCK: end = "stuck"
            elif last[5] < P.TOL: end = "tol"
        elif tr[0, c, 5] < P.TOL: end = "tol"
        out.append(dict(steps=steps, end=end, trials=[int(tr[k, c, 3]) for k in steps]))
    return out


# ---- graphs of the stage tests (n, ii, jj sorted, 0-based)
def wheel(n):
    """Hub last (node n - 1), a ring on the rim 0 .. n - 2."""
    r = n - 1
    e = [(k, k + 1) for k in range(r - 1)] + [(0, r - 1)] + [(k, r) for k in range(r)]
    e = np.array(sorted(e), dtype=np.int64)
    return n, e[:, 0].copy(), e[:, 1].copy()


def small_graph(n):
    """A path 0 - 1 - ... - n - 1 with the chord (0, n - 1) when n > 2."""
    e = [(k, k + 1) for k in range(n - 1)] + ([(0, n - 1)] if n > 2 else [])
    e = np.array(sorted(set(e)), dtype=np.int64)
    return n, e[:, 0].copy(), e[:, 1].copy()


def stage_shapes():
    """name -> (n, ii, jj): the shapes every stage runs on."""
    def make():
        out = {"edge": K.path_graph(1)}
        for m in (255, 256, 257):
            out[f"path{m}"] = K.path_graph(m)
        for sp in (15, 16, 17, 33):
            out[f"star{sp}-hub0"] = K.star_graph(sp, False); out[f"star{sp}-hub-last"] = K.star_graph(sp, True)
        for n in (3, 4, 5, 17):
            out[f"n{n}"] = small_graph(n)
        out["k363"] = K.complete_graph(363)
        out["wheel65600"] = wheel(65600)
        return {k: (int(v[0]), np.asarray(v[1], dtype=np.int64), np.asarray(v[2], dtype=np.int64)) for k, v in out.items()}
    return _once("shapes", make)


def synthetic_state(n, m, seed):
    """Finite data of mixed sign and scale in every array, in the solver's sign pattern where the formulas divide (fu < 0 < lamu), row 0
    of the node arrays non-zero (so that a write to it shows), -> (state, scal)."""
    g = np.random.default_rng(seed)

    def mixed(shape):
        return g.choice([-1.0, 1.0], size=shape) * 10.0 ** g.uniform(-3, 3, size=shape)
    st = {k: mixed((m, 3)) for k in P.EDGE}
    st.update({k: mixed((n, 3)) for k in P.NODE})
    for k in ("f1", "f2"):
        st[k] = -np.abs(st[k])
    for k in ("l1", "l2", "u", "s1", "sx"):
        st[k] = np.abs(st[k])
    scal = dict(tau=10.0 ** g.uniform(0, 3, size=3), s=g.uniform(0.05, 0.99, size=3), ymax=10.0 ** g.uniform(-1, 1, size=3), act=(1, 1, 1))
    return st, scal

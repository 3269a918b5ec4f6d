"""TEST INFRASTRUCTURE -- the cases and the integer reference of the mirror column sums (k_colsum_node, desc_amd/csrc/pgd.hip;
DESC_PGD.m:185-191).

The kernel adds 64-bit fixed-point integers, round(w * 2^fx_bits) with fx_bits = 62 - ceil(log2(max degree + 1)): what it must
produce is an integer that NumPy computes exactly, so tests/test_gpu_colsum.py compares with ``np.array_equal`` and no tolerance.
tests/test_colsum_reference_host.py checks this reference against the plain double sums and re-asserts, on the CPU, the
structural facts for which each case is in the table.

Names: the oracle structure ``st`` (oracle.build_structure) has segment l = edge pos_edge[l] = (i, j), i < j, with the cycles
cum_ind[l] .. cum_ind[l + 1]; ikj[c] / jki[c] = the mirror cycle ({i,k}; j) / ({j,k}; i) of cycle c = ({i,j}; k), -1 if it was not
sampled.  "nact" = contributing cycles of a segment at one endpoint = the cycles of the segment whose mirror at that endpoint was
sampled (the mirror relation is symmetric), i.e. count(ikj >= 0) at i and count(jki >= 0) at j."""
import numpy as np

from desc_amd.algorithms import marshal_edges
from tests import graph_shapes as G
from tests.helpers import csr, make_problem

MAX_SEG_CYCLES = 256          # desc_amd/csrc: the longest segment of the node layout
COLSUM_SHORT = 128            # ... rows with at most this many owned segments take the wave-per-node path on a shard


def _er(n, p):
    return lambda: make_problem("uniform", n=n, p=p, q=0.2, sigma=0.1, seed=8)[1:]


def _shape(mo):
    nn, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None
    return nn, ii, jj, rij


def _complete(n):
    return lambda: _shape(G.band(n, n - 1, seed=n))            # i ~ i +- 1 .. +- (n - 1): every pair


# name -> graph, n_sample_min, structure seed, worlds, host or device structure builder (the column-index streams are made by other kernels
# after each), what the case is there for.  *_full: codegree <= n_sample_min everywhere, so every mirror of every cycle was sampled.
CASES = {
    "triangle": dict(graph=_complete(3), nmin=30, seed=0, worlds=(1,), where="host",
                     why="max_deg + 1 = 3, fx_bits = 60, every column = 2^60"),
    "K64": dict(graph=_complete(64), nmin=64, seed=0, worlds=(1, 2), where="device",
                why="max_deg + 1 = 64, an exact power of two: fx_bits = 56; nact = 62"),
    "er40": dict(graph=_er(40, 0.5), nmin=30, seed=3, worlds=(1, 2, 3), where="device",
                 why="segment lengths 3..20, 8 lanes by rule, 6 segments with nact > 16 take a second round"),
    "er200": dict(graph=_er(200, 0.8), nmin=30, seed=3, worlds=(1, 3, 8), where="device",
                  why="8 lanes by rule; nact <= 20"),
    "er60_full": dict(graph=_er(60, 0.9), nmin=100, seed=3, worlds=(1, 2), where="device",
                      why="all mirrors sampled; nact 39..56: 2 rounds at 16 lanes, 4 at 8"),
    "er150_full": dict(graph=_er(150, 0.9), nmin=100, seed=3, worlds=(1, 3), where="device",
                       why="nact up to 97: 4 rounds at 16 lanes, 7 at 8"),
    "K258": dict(graph=_complete(258), nmin=256, seed=0, worlds=(1, 3), where="host", states=("distinct", "collapsed"),
                 why="every segment has 256 = MAX_SEG_CYCLES contributing cycles: the last round of both instances, bit 8 of the count "
                     "field; rows of 257 slots, one past the 256-thread stride"),
    "bridged150_60": dict(graph=lambda: _shape(G.model("bridged150_60")), nmin=30, seed=0, worlds=(1, 2), where="host",
                          why="edges without cycles inside rows: zero-length runs"),
    "hub1500_mid": dict(graph=lambda: _shape(G.model("hub1500_mid")), nmin=30, seed=0, worlds=(1, 2, 3, 8), where="host",
                        why="max_deg = 1499: fx_bits = 51; one row longer than 128, every other row on the wave-per-node path of a shard; "
                            "columns beyond 1024"),
}
# the weight states: iterations, step, (patience stays at its default 30: the stop rule cannot fire within 10 iterations)
STATES = {
    "uniform": dict(iters=0, lr=0.01),           # w = 1 / cnt: rint(2^fx / cnt) for counts that are no powers of two (inexact where 1 / cnt < 2^(52 - fx))
    "distinct": dict(iters=2, lr=0.001),         # every cycle a weight of its own
    "collapsed": dict(iters=10, lr=1.0),         # mostly exact zeros and exact ones: the largest column sums
}
DISTINCT_LR = {"K258": 0.0005}                   # at 0.001 only 99.2 % of K258's cycles are distinguishable (CPU oracle)


def states_of(case):
    return CASES[case].get("states", tuple(STATES))


def step_of(case, state):
    s = dict(STATES[state])
    if state == "distinct":
        s["lr"] = DISTINCT_LR.get(case, s["lr"])
    return s


_graphs, _structs = {}, {}


def graph(case):
    """(nn, ii, jj, rij) of a case, built once per process."""
    if case not in _graphs:
        _graphs[case] = CASES[case]["graph"]()
    return _graphs[case]


def structure(oracle, case):
    """The oracle's cycle structure of a case, built once per process and never changed."""
    if case not in _structs:
        nn, ii, jj, rij = graph(case)
        _structs[case] = oracle.build_structure(nn, ii, jj, seed=CASES[case]["seed"], n_sample_min=CASES[case]["nmin"])
    return _structs[case]


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def max_degree(nn, ii, jj):
    return int(np.bincount(np.concatenate([ii, jj]), minlength=nn).max())


def fx_bits_of(max_deg):
    """prepare_colsum: 62 - (the smallest b with 2^b >= max_deg + 1)."""
    b = 0
    while (1 << b) < max_deg + 1:
        b += 1
    return 62 - b


def quantize(w, fx_bits):
    """round(w * 2^fx_bits), half to even as __double2ll_rn; the scaling by a power of two is exact."""
    return np.rint(np.ldexp(np.asarray(w, dtype=np.float64), fx_bits)).astype(np.int64)


def seg_of_cycle(st):
    return np.repeat(np.arange(st["m_pos"], dtype=np.int64), np.diff(st["cum_ind"]))


def uniform_weights(st):
    """k_init_node: w = 1.0 / (double)cnt for every cycle of a segment of cnt cycles."""
    return (1.0 / np.diff(st["cum_ind"]).astype(np.float64))[seg_of_cycle(st)]


def mirror_sums(st, q, owned=None):
    """(T1, T2), int64 per segment: T1[l] = sum of q[ikj[c]] over the cycles c of segment l with ikj[c] >= 0 (CSR slot (row i, column j)),
    T2[l] the same with jki (slot (row j, column i)).  owned (bool per segment): only the mirror cycles that lie in an owned segment --
    one rank's partial sums."""
    seg = seg_of_cycle(st)
    out = []
    for key in ("ikj", "jki"):
        idx = np.asarray(st[key], dtype=np.int64)
        ok = idx >= 0
        if owned is not None:
            ok &= owned[seg[np.where(ok, idx, 0)]]
        T = np.zeros(st["m_pos"], dtype=np.int64)
        np.add.at(T, seg[ok], q[idx[ok]])
        out.append(T)
    return out


def mirror_counts(st):
    """(nact at i, nact at j) per segment: the number of terms of T1 / T2."""
    seg = seg_of_cycle(st)
    return [np.bincount(seg[np.asarray(st[key]) >= 0], minlength=st["m_pos"]).astype(np.int64) for key in ("ikj", "jki")]


def edge_slots(nn, ii, jj):
    """CSR slot (row i, column j) and slot (row j, column i) of every edge (i < j), in the library's CSR order."""
    rowptr, adj, adj_eid, row_of = csr(nn, ii, jj)
    up = np.empty(ii.shape[0], dtype=np.int64); dn = np.empty(ii.shape[0], dtype=np.int64)
    upper = adj > row_of
    up[adj_eid[upper]] = np.flatnonzero(upper)
    dn[adj_eid[~upper]] = np.flatnonzero(~upper)
    return up, dn


def per_slot(st, nn, ii, jj, T1, T2):
    """The sums per CSR slot (2m of them): slots of edges without cycles are 0."""
    up, dn = edge_slots(nn, ii, jj)
    pe = np.asarray(st["pos_edge"], dtype=np.int64)[:st["m_pos"]]
    out = np.zeros(2 * ii.shape[0], dtype=np.int64)
    out[up[pe]] = T1
    out[dn[pe]] = T2
    return out


def contributing(st):
    """The cycles whose weight the column sums read: those that are somebody's sampled mirror."""
    idx = np.concatenate([np.asarray(st["ikj"]), np.asarray(st["jki"])])
    return np.unique(idx[idx >= 0])


def distinct_fraction(st, w):
    """Share of the contributing cycles whose weight no other cycle of their segment carries: a column index paired with the wrong cycle of
    the same segment then changes T."""
    seg = seg_of_cycle(st)
    w = np.asarray(w, dtype=np.float64)
    order = np.lexsort((w, seg))
    s, v = seg[order], w[order]
    same_next = np.zeros(order.size, dtype=bool); same_next[:-1] = (s[1:] == s[:-1]) & (v[1:] == v[:-1])
    dup_sorted = same_next.copy(); dup_sorted[1:] |= same_next[:-1]
    dup = np.empty(order.size, dtype=bool); dup[order] = dup_sorted
    c = contributing(st)
    return 1.0 if c.size == 0 else float(np.count_nonzero(~dup[c])) / c.size


def rounds(nact_max, cl):
    """Rounds colsum_walk takes for a segment end of nact contributing cycles at cl lanes per segment (2 cl slots a round)."""
    return max(1, -(-int(nact_max) // (2 * cl)))

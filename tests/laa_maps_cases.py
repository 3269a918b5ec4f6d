"""Inputs of the per-kernel tests of the Lie-algebraic averaging core, shared by tests/test_laa_maps_host.py (which checks the references
on them, without a GPU) and tests/test_gpu_laa_maps.py (which runs the kernels on them).  Each builder returns the smallest arrays that
reach the branches the kernel text has; the table in tests/test_gpu_laa_maps.py maps them to kernel lines."""
import mpmath as mp
import numpy as np

PI = np.pi
THETAS = [2.0 ** -30, 1e-8, 1.0, PI / 2, PI - 1e-3, PI - 1e-6, PI - 1e-8]


def rng(seed):
    return np.random.default_rng(seed)


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def rot(axis, theta):
    """Rodrigues' formula in double -> 9 doubles column-major."""
    n = unit(axis)
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    R = np.eye(3) + np.sin(theta) * K + (1 - np.cos(theta)) * (K @ K)
    return R.reshape(9, order="F")


def axes():
    g = rng(11)
    return [np.eye(3)[k] for k in range(3)] + [unit(g.normal(size=3)) for _ in range(20)]


def colmajor(Mx):
    return np.asarray(Mx, dtype=np.float64).reshape(9, order="F")


def path_graph(m):
    """Edges (k, k + 1), k < m: m + 1 nodes, sorted."""
    return m + 1, np.arange(m, dtype=np.int32), np.arange(1, m + 1, dtype=np.int32)


def star_graph(spokes, hub_last):
    n = spokes + 1
    if hub_last:
        return n, np.arange(spokes, dtype=np.int32), np.full(spokes, n - 1, dtype=np.int32)
    return n, np.zeros(spokes, dtype=np.int32), np.arange(1, n, dtype=np.int32)


def grid_graph(k):
    e = []
    for r in range(k):
        for c in range(k):
            v = r * k + c
            if c + 1 < k: e.append((v, v + 1))
            if r + 1 < k: e.append((v, v + k))
    e.sort()
    e = np.array(e, dtype=np.int32)
    return k * k, e[:, 0].copy(), e[:, 1].copy()


def complete_graph(n):
    e = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], dtype=np.int32)
    return n, e[:, 0].copy(), e[:, 1].copy()


def identity_rij(m):
    return np.tile(np.eye(3).reshape(9), (m, 1))


# ---------------------------------------------------------------------------------------------------------------- r2q / q2r
def near_pi_rotations():
    return np.array([rot(a, t) for t in (PI - 1e-3, PI - 1e-6, PI - 1e-8) for a in axes()[:6]])


def r2q_blocks():
    """-> (R (N, 9), labels, well: theta <= pi - 1e-3 rotations, for the round trip)."""
    R, lab, well = [np.eye(3).reshape(9)], ["identity"], [True]
    for t in THETAS:
        for k, a in enumerate(axes()):
            R.append(rot(a, t)); lab.append(f"theta={t:.3g} axis{k}"); well.append(t <= PI - 1e-3)
    for d in ([1, -1, -1], [-1, 1, -1], [-1, -1, 1]):                      # exact half-turns: a = 0, R2Q.m:12 divides by it
        R.append(colmajor(np.diag(d))); lab.append(f"half-turn diag{d}"); well.append(False)
    n = unit(rng(12).normal(size=3))
    R.append(colmajor(2 * np.outer(n, n) - np.eye(3))); lab.append("half-turn random axis"); well.append(False)
    nan_b = np.eye(3).reshape(9).copy(); nan_b[1] = np.nan
    inf_b = np.eye(3).reshape(9).copy(); inf_b[5] = np.inf
    two = colmajor(rot([1, 2, 3], 0.7).reshape(3, 3, order="F") @ np.diag([2.0, 1.0, 1.0]) @ rot([3, -1, 2], 1.1).reshape(3, 3, order="F"))
    for b, l in ((np.zeros(9), "zero"), (2 * np.eye(3).reshape(9), "2I"), (-np.eye(3).reshape(9), "-I (sqrt of a negative)"), (nan_b, "one NaN"),
                 (inf_b, "one Inf"), (two, "projection output with round(S) = 2")):
        R.append(b); lab.append(l); well.append(False)
    return np.array(R), lab, np.array(well)


R2Q_COUNTS = [1, 255, 256, 257, 512 * 256 + 5]            # the last wraps the grid-stride loop of the node grid (at most 512 blocks)


def tiled(a, count):
    a = np.asarray(a)
    reps = -(-count // a.shape[0])
    return np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:count]


def q2r_quats():
    g = rng(13)
    Q = []
    for a in (1.0, 1 - 1e-13, 1 - 1e-12, 1 - 2e-12):                       # both sides of q2R.m:4's 1e-12
        for s in (1.0, -1.0):
            v = unit(g.normal(size=3)) * np.sqrt(max(0.0, 1 - a * a))
            Q.append([s * a, *v])
    Q.append([0.0, *unit(g.normal(size=3))])                               # half-turn
    Q.append([-0.0, 0.0, 1.0, 0.0])
    Q.append([0.0, 0.0, 0.0, 0.0])                                         # s2 = 0: 0/0
    Q.append([0.5, 0.0, 0.0, 0.0])                                         # s2 = 0 away from |a| = 1
    for sc in (0.5, 2.0, 1e-3):                                            # unnormalised: q2R.m does not renormalise
        q = unit(g.normal(size=4)); Q.append(list(sc * q))
    for _ in range(8):
        Q.append(list(unit(g.normal(size=4))))
    Q.append([np.nan, 0.0, 0.0, 1.0]); Q.append([0.3, np.inf, 0.0, 0.0])
    return np.array(Q)


# ---------------------------------------------------------------------------------------------------------------- edge_log
def edge_log_control():
    """A path whose node quaternions alternate (1,0,0,0), (-1,0,0,0): both products of k_edge_log are then exact and the residual
    quaternion v of edge e IS QQ[e].  -> (n, ii, jj, Q, QQ = the wanted v's, labels, expected sign of B . axis or 0)."""
    g = rng(14)
    V, lab, sign, ax = [], [], [], []

    def add(a, vec, label, sg):
        V.append([a, *vec]); lab.append(label); sign.append(sg); ax.append(unit(vec) if np.linalg.norm(vec) > 0 else np.zeros(3))

    add(1.0, [0, 0, 0], "v = (1,0,0,0): s2 = 0, 0/0 -> 0", 0)
    add(-1.0, [0, 0, 0], "v = (-1,0,0,0): 2 atan2(0,-1) = 2 pi wraps to 0", 0)
    add(1.0, [1e-160, 0, 0], "s2 = 1e-160 (s2^2 underflows)", +1)
    add(1.0, [6e-161, 8e-161, 0], "s2 = 1e-160, two components", +1)
    for k in range(3):
        n = unit(g.normal(size=3)); add(np.cos(5e-9), np.sin(5e-9) * n, "angle 1e-8", +1)
    for d in (1e-9, 1e-3):
        for sg in (-1, +1):                                                # angle pi + sg d: below pi -> +, above -> wraps to -(pi - d)
            n = unit(g.normal(size=3)); phi = PI + sg * d
            add(np.cos(phi / 2), np.sin(phi / 2) * n, f"angle pi{'+' if sg > 0 else '-'}{d:g}", -sg)
    n = unit(g.normal(size=3)); add(-0.5, np.sqrt(0.75) * n, "v.a < 0, large s2", -1)
    n = unit(g.normal(size=3)); add(-0.9, np.sqrt(0.19) * n, "v.a < 0", -1)
    knife = len(V)
    add(0.0, [0.0, 1.0, 0.0], "v.a = +0, s2 = 1: knife edge", None)
    add(-0.0, [0.0, 1.0, 0.0], "v.a = -0, s2 = 1: knife edge", None)
    add(0.0, [0.6, 0.0, 0.8], "v.a = +0, s2 = 1 (0.6, 0.8): knife edge", None)
    for k in range(6):
        q = unit(g.normal(size=4)); add(q[0], q[1:], "random", None)
    m = len(V)
    n_nodes, ii, jj = path_graph(m)
    Q = np.zeros((n_nodes, 4)); Q[:, 0] = np.where(np.arange(n_nodes) % 2 == 0, 1.0, -1.0)
    return dict(n=n_nodes, ii=ii, jj=jj, Q=Q, QQ=np.array(V), labels=lab, sign=sign, axis=np.array(ax), knife=[knife, knife + 1, knife + 2])


def edge_log_random():
    """Random unit quaternions on a complete graph of 9 nodes (gathers by i and j that are not e and e + 1) and on a path of 300."""
    out = []
    for k, (n, ii, jj) in enumerate((complete_graph(9), path_graph(300))):
        g = rng(15 + k)
        Q = np.array([unit(g.normal(size=4)) for _ in range(n)]); QQ = np.array([unit(g.normal(size=4)) for _ in range(len(ii))])
        out.append(dict(n=n, ii=ii, jj=jj, Q=Q, QQ=QQ))
    return out


# ---------------------------------------------------------------------------------------------------------------- rhs
def rhs_cases():
    out = []
    for name, (n, ii, jj) in (("star17 hub 0", star_graph(17, False)), ("star33 hub 0", star_graph(33, False)), ("star17 hub last", star_graph(17, True)),
                              ("star33 hub last", star_graph(33, True)), ("path 40", path_graph(39)), ("grid 5x5", grid_graph(5))):
        g = rng(len(name) * 7 + n)
        m = len(ii)
        B = g.normal(size=(m, 3))
        for wname, w in (("ones", np.ones(m)), ("1e-4 | 1e4", np.where(np.arange(m) % 2 == 0, 1e-4, 1e4)), ("loguniform", 10.0 ** g.uniform(-4, 4, size=m))):
            out.append(dict(name=f"{name}, w {wname}", n=n, ii=ii, jj=jj, w=w, B=B))
        w = np.ones(m); iso = 1 if "hub last" in name else n - 1
        w[(ii == iso) | (jj == iso)] = 0.0                                   # every edge of one node has weight 0: diag = 0 there
        out.append(dict(name=f"{name}, node {iso} isolated", n=n, ii=ii, jj=jj, w=w, B=B, iso=iso))
    return out


# ---------------------------------------------------------------------------------------------------------------- pcg
def pcg_graphs():
    return [("edge", path_graph(1)), ("path40", path_graph(39)), ("grid5x5", grid_graph(5)), ("star17 hub0", star_graph(17, False)),
            ("star17 hublast", star_graph(17, True)), ("K12", complete_graph(12))]


def pcg_cases():
    """Weighted_LAA's instance (<false,false>, probe 25): graph x weights with a random right-hand side, and on two graphs the zero /
    one-coordinate-zero right-hand sides and the act masks."""
    out = []
    for gname, (n, ii, jj) in pcg_graphs():
        m = len(ii); g = rng(100 + n + m)
        iso = None if gname == "edge" else (1 if "hublast" in gname else n - 1)
        weights = [("ones", np.ones(m), None), ("loguniform", 10.0 ** g.uniform(-4, 4, size=m), None)]
        if iso is not None:
            w = np.ones(m); w[(ii == iso) | (jj == iso)] = 0.0
            weights.append(("isolated", w, iso))
        for wname, w, iso_v in weights:
            rhs = g.normal(size=(n, 3))
            if iso_v is not None: rhs[iso_v] = 0.0                          # as k_rhs gives it: no weight, no right-hand side
            out.append(dict(name=f"{gname} {wname} random", n=n, ii=ii, jj=jj, w=w, rhs=rhs, act=(1, 1, 1)))
        if gname in ("edge", "grid5x5", "path40"):
            w = np.ones(m); rhs = g.normal(size=(n, 3))
            out.append(dict(name=f"{gname} zero rhs", n=n, ii=ii, jj=jj, w=w, rhs=np.zeros((n, 3)), act=(1, 1, 1), zero=True))
            r1 = rhs.copy(); r1[:, 1] = 0.0
            out.append(dict(name=f"{gname} rhs zero in y", n=n, ii=ii, jj=jj, w=w, rhs=r1, act=(1, 1, 1)))
            for act in ((1, 0, 0), (0, 1, 1)):
                out.append(dict(name=f"{gname} act {act}", n=n, ii=ii, jj=jj, w=w, rhs=rhs, act=act))
    for c in out:
        c["diag"] = diag_of(c["n"], c["ii"], c["jj"], c["w"] * c["w"])
    return out


def diag_of(n, ii, jj, wc):
    d = np.zeros(n)
    np.add.at(d, ii, wc); np.add.at(d, jj, wc)
    return d


def pcg3_cases():
    """The primal-dual instance (<true,true>, probe 5): one weight per edge and coordinate, the Jacobi diagonal per node and coordinate with
    row 0 = 0 (k_pd_gather<2>)."""
    out = []
    for gname, (n, ii, jj) in pcg_graphs():
        m = len(ii); g = rng(200 + n + m)
        w = 10.0 ** g.uniform(-2, 2, size=(m, 3)); rhs = g.normal(size=(n, 3))
        out.append(dict(name=f"{gname} w3 random", n=n, ii=ii, jj=jj, w=w, rhs=rhs, act=(1, 1, 1)))
        if gname in ("grid5x5", "K12"):
            out.append(dict(name=f"{gname} w3 zero rhs", n=n, ii=ii, jj=jj, w=w, rhs=np.zeros((n, 3)), act=(1, 1, 1), zero=True))
            w0 = w.copy(); w0[:, 1] = 0.0                                    # pq = 0, rz = 0: the coordinate never moves
            out.append(dict(name=f"{gname} w3 y weights 0, act (1,0,1)", n=n, ii=ii, jj=jj, w=w0, rhs=rhs, act=(1, 0, 1), dead=1))
            wn = w.copy(); wn[m // 2, 2] = np.nan                            # breakdown: back in bad[2], x and y solved
            out.append(dict(name=f"{gname} w3 NaN weight in z", n=n, ii=ii, jj=jj, w=wn, rhs=rhs, act=(1, 1, 1), nan=2))
    for c in out:
        d = np.stack([diag_of(c["n"], c["ii"], c["jj"], c["w"][:, k]) for k in range(3)], axis=1); d[0] = 0.0
        c["diag"] = d; c["w3"] = True
    return out


def pcg_cap_case():
    """NaN-free and unable to converge: a zero Jacobi diagonal keeps z = p = 0, so alpha = 0 and r = b at every step; the single-edge
    graph stops at the cap min(20000, 20 n + 200) = 240."""
    n, ii, jj = path_graph(1)
    return dict(name="edge, diag 0: cap", n=n, ii=ii, jj=jj, w=np.ones(1), rhs=np.array([[0.0, 0, 0], [1.0, -2.0, 3.0]]), diag=np.zeros(2), act=(1, 1, 1))


# ---------------------------------------------------------------------------------------------------------------- node update
def node_update_base():
    """40 rows: row 0 non-zero (moves Q[0], does not count in the score), the theta list, a NaN row, random rows."""
    g = rng(16)
    rows = [0.3 * unit(g.normal(size=3))]
    for th in (0.0, 1e-200, 1e-160, 1e-8, 1.0, PI, 2 * PI, 10.0):
        rows.append(th * unit(g.normal(size=3)) if th else np.zeros(3))
    rows.append([1e-200, 0.0, 0.0]); rows.append([0.0, 1e-160, 0.0]); rows.append([-0.0, 0.0, -0.0])
    rows.append([np.nan, 0.1, 0.2])
    while len(rows) < 40:
        rows.append(g.uniform(0, 2) * unit(g.normal(size=3)))
    x = np.array(rows, dtype=np.float64)
    Q = np.array([unit(g.normal(size=4)) for _ in range(len(rows))])
    return x, Q


NODE_COUNTS = [1, 255, 256, 257, 64 * 256 + 3]


# ---------------------------------------------------------------------------------------------------------------- weights
def weights_values():
    """RS values; the crossing of 1 / x^0.75 with 1e4 is computed at 50 digits."""
    mp.mp.dps = 50
    xc = float(mp.power(mp.mpf(10), mp.mpf(-16) / 3))
    cross = [xc]
    for k in range(3):
        cross = [np.nextafter(cross[0], 0.0)] + cross + [np.nextafter(cross[-1], 1.0)]
    g = rng(17)
    vals = [0.0, -0.0, 1e-320, 5e-324, 1e-300, *cross, 0.5, np.nextafter(0.5, np.inf), np.nextafter(0.5, 0.0), 1.0, 3.0, 1e300, np.inf, np.nan, -1.0,
            -1e-320, -np.inf, *g.uniform(0, 1, size=40), *(10.0 ** g.uniform(-12, 3, size=40))]
    return np.array(vals, dtype=np.float64)


WEIGHT_THRESHOLDS = [0.5, np.inf, -np.inf, np.nan, 0.0]


def irls_weight_cases():
    n, ii, jj = path_graph(60)
    g = rng(18)
    x = 0.1 * g.normal(size=(n, 3)); B = 0.1 * g.normal(size=(60, 3))
    x[0] = [5.0, -7.0, 9.0]                                                 # node 0 is grounded: its row must not be read as a value
    x[10:13] = 0.0; B[10:12] = 0.0                                          # s = 0 on edges 10, 11
    B[20] = x[21] - x[20]                                                   # s = 0 by cancellation
    return dict(n=n, ii=ii, jj=jj, x=x, B=B, sigmas=[5 * PI / 180, 1e-300, 1e-170, 1e200, 1e160])


# ---------------------------------------------------------------------------------------------------------------- quantile
Q_SIZES = [1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 70001]


def quantile_ps(m):
    return [0.0, 0.5 / m, np.nextafter(0.5 / m, 1.0), 0.3, 0.5, 0.8, 0.9, 1 - 0.5 / m, 1.0]


def p_for_rank(m, k0, fr):
    """p whose Hazen position p m + 0.5 has 0-based lower rank k0 and fraction about fr."""
    return (k0 + 0.5 + fr) / m


def quantile_data():
    """-> list of (name, x, list of p)."""
    g = rng(19)
    out = []
    for m in Q_SIZES:
        out.append((f"uniform m={m}", g.uniform(0, 1, size=m), quantile_ps(m)))
    for m in (3, 257, 4097):
        ps = quantile_ps(m)
        out.append((f"constant m={m}", np.full(m, 0.37), ps))
        out.append((f"two values m={m}", np.where(g.uniform(size=m) < 0.4, -1.5, 2.25), ps))
        x = g.uniform(0, 1, size=m); x[: (9 * m) // 10] = 0.5; g.shuffle(x)
        out.append((f"90% ties m={m}", x, ps))
        out.append((f"negative m={m}", -10.0 ** g.uniform(-3, 3, size=m), ps))
        out.append((f"1e-300..1e300 m={m}", 10.0 ** g.uniform(-300, 300, size=m), ps))
        x = g.normal(size=m) * 1e3; x[0] = -1e308; x[1] = 1e308
        out.append((f"hi - lo overflows m={m}", x, [p for p in ps if 1.5 / m < p < 1 - 1.5 / m]))
    # exact bin layouts: integers 0..4095 alone occupy a bin each (adjacent bins); with the outlier 1e6 the bins are 244.14 wide
    ints = np.arange(4096, dtype=np.float64)
    out.append(("ints 0..4095: adjacent bins", g.permutation(ints), [p_for_rank(4096, k, 0.25) for k in (0, 1, 2047, 4093, 4094)] + quantile_ps(4096)))
    x = g.permutation(np.append(ints, 1e6))
    out.append(("ints + outlier: same bin / last of its bin", x, [p_for_rank(4097, k, 0.75) for k in (100, 243, 244, 245, 488, 489, 4094, 4095)]))
    x = g.permutation(np.concatenate([np.arange(100.0), 1e6 + np.arange(100.0)]))
    out.append(("two clusters: thousands of empty bins between", x, [p_for_rank(200, k, 0.3) for k in (98, 99, 100)]))
    return out


QUANTILE_CAPS = [1 << 20, 8, 1]                       # the library's own capacity (QCAP in laa.hip, _lib.HOOK_QCAP), then two that force the host path


# ---------------------------------------------------------------------------------------------------------------- projection
S_LIST = [0.4999, 0.5, 0.5001, 0.9, 0.91, 0.99, 0.991, 1.0, 1.009, 1.1, 1.4999, 1.5, 2.4]


def _m3(b):
    return np.asarray(b).reshape(3, 3, order="F")


def project_good_blocks():
    """Blocks every status of which is decided (no singular value within 1e-12 of a threshold) and >= 0 warnings, no failure."""
    g = rng(20)
    out = [np.eye(3).reshape(9)] + [rot(a, t) for t in THETAS for a in axes()[:4]] + list(near_pi_rotations())
    for s in (0.4999, 0.5001, 0.91, 0.991, 1.009, 1.4999, 2.4):               # one and two positions: status 0 while one value is near 1
        for pos in ([0], [0, 1]):
            d = np.ones(3); d[pos] = s
            out.append(colmajor(_m3(rot(g.normal(size=3), 0.9)) @ np.diag(d) @ _m3(rot(g.normal(size=3), 2.1))))
    for s in (0.95, 1.05, 0.985, 1.02):                                       # all three off 1 by >= 0.01 and < 0.1: warned
        out.append(colmajor(s * _m3(rot(g.normal(size=3), 1.3))))
    out.append(colmajor(_m3(rot(g.normal(size=3), 0.4)) @ np.diag([1.05, 0.95, 1.03]) @ _m3(rot(g.normal(size=3), 0.2))))
    return np.array(out)


def project_bad_blocks():
    """Failing blocks: reflections (det < 0 -> 3), all three singular values off 1 by >= 0.1 (-> 2), rank-deficient ones (det ~ 0)."""
    g = rng(21)
    out = []
    out.append(colmajor(np.diag([1.0, 1.0, -1.0])))                           # reflection
    out.append(colmajor(-_m3(rot(g.normal(size=3), 0.8))))                    # reflection
    for s in (0.4999, 0.5001, 1.1001, 1.4999, 2.4, 0.8):
        out.append(colmajor(s * _m3(rot(g.normal(size=3), 1.7))))             # all three positions
    out.append(np.zeros(9))                                                    # det exactly 0, s = 0 skipped
    u, v = unit(g.normal(size=3)), unit(g.normal(size=3))
    out.append(colmajor(np.outer(u, v)))                                       # rank 1
    out.append(colmajor(np.diag([1.0, 1.0, 0.0])))                             # rank 2, det exactly 0
    out.append(colmajor(_m3(rot(g.normal(size=3), 0.5)) @ np.diag([1.0, 0.7, 0.0])))
    return np.array(out)


def project_knife_blocks():
    """Singular values ON the thresholds: exact ones (signed permutations times diag(s): the Jacobi SVD of orthogonal columns is exact)
    and rotated ones (decided only where NumPy's singular values are farther than 1e-12 from a threshold)."""
    g = rng(22)
    perm = np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])                      # a rotation
    out, exact = [], []
    for s in S_LIST:
        for pos in ([0], [0, 1], [0, 1, 2]):
            d = np.ones(3); d[pos] = s
            out.append(colmajor(perm @ np.diag(d))); exact.append(True)
            out.append(colmajor(_m3(rot(g.normal(size=3), 0.9)) @ np.diag(d) @ _m3(rot(g.normal(size=3), 2.1)))); exact.append(False)
    for d in ([2.0, 2.0, 1.0], [1.0, 1.0, 1.0], [1.2, 1.2, 1.2], [3.0, 1.0, 1.0]):     # repeated singular values
        out.append(colmajor(_m3(rot(g.normal(size=3), 0.3)) @ np.diag(d) @ _m3(rot(g.normal(size=3), 1.1)))); exact.append(False)
    return np.array(out), np.array(exact)

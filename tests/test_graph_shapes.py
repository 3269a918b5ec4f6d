"""Qualifies the table of tests/graph_shapes.py on the CPU, so that a red case of tests/test_gpu_graph_shapes.py means the kernel is
wrong and not that the graph is ill-conditioned or has drifted off the branch it was made for.

* Every threshold is read out of the sources by regex; every side of every branch below is claimed by a shape, and every shape lies
  on the sides it claims (plain NumPy from ``Ind``).  Changing a constant in a kernel fails this file instead of dropping coverage.
* Every shape but ``two_components`` is connected.
* Every oracle the GPU file compares against is run twice on every shape it is used on: as is, and with ``RijMat`` (and ``S_vec``
  where it is an input) scaled entrywise by 1 + 2.2e-16 {-1, 0, 1}.  The oracle must not move by more than 1/100 of the tolerance the
  GPU test applies (the method of tests/test_gpu_irls.py's docstring and tests/test_irls_host.py).
* A NumPy Jacobi-PCG with the operator, stop and cap of desc_amd/csrc/laa.hip finishes within half the cap on the weights and
  right-hand sides of the first and of the fifth (the first 0.8-quantile) step of the refinement oracle, run for exactly five steps
  on every shape the refinement, MPLS or IRLS use: ``cg_unconverged == 0`` is a fair demand on the GPU.
* The refinement and MPLS oracles run at least 4 steps on their shapes, so the quantile threshold really moves.

Measured on the CPU with the oracles (never with the library); every test prints its figures before it asserts (``pytest -s``).
QUALIFIED: the worst movement per oracle over the shapes of the table, next to the bound (1/100 of the GPU tolerance):

    CEMP SVec        8.4e-15  power_law500    (1e-14)      Spectral          3.6e-13  bridged150_60   (1e-10)
    GCW              1.1e-12  bridged150_60   (1e-10)      refinement R_est  2.0e-13  band200_10      (1e-9)
    MPLS R_est       3.7e-10  bridged150_60   (1e-9)       MPLS R_init       2.0e-15                  (1e-12)
    IRLS R           2.8e-12  power_law200    (1e-9)       IRLS R_l1         1.1e-12  power_law200    (1e-11)
    CEMP, unbatched  3.0e-15  hub40_mid, nsample 64 .. 300 (1e-14)  PGD S_vec  8.8e-13  hub1500_mid     (1e-12)
    LP, 50 steps     5.5e-15  hub100_mid      (1e-14)      MST, two multiplication orders along 5000 products  9.9e-15 (1e-14)
    Jacobi-PCG       267 of 10200 iterations (power_law500, 0.8-quantile weights); hubs 39-189 of 3200 / 8200, bands 93-143 of 4200

Not perturbed: the S_vec that the GCW cases take from the PGD oracle.  There S_vec is an input that the device and gcw_oracle both
receive, so the PGD oracle's conditioning does not enter the comparison; gcw_oracle's own sensitivity to S_vec is measured with the
synthetic S_vec, perturbed.  The sweep cases also compare S0 at 1e-14 (tests/test_gpu_sweep_instances.py); that one is not qualified.

Shapes that were tried and replaced because an oracle moved too much on them (the bound was never widened):
  * CEMP with Haar outliers (q = 0.2, 0.3).  A cycle through an outlier has a Haar-distributed angle, within 1e-4 of pi for one cycle
    in ~1e4, and acos((trace - 1) / 2) there turns 1 ulp of the trace into 1e-12 of S0: the oracle moved by 4e-14 (hub n = 300) to
    9.7e-12 (hub n = 8300, an edge with one common neighbour and S0 = 0.9999967) -- above the 1e-12 tolerance itself.  Without
    outliers (q = 0, sigma = 0.2 .. 0.3) what is left is the amplification of the six reweighting rounds (beta up to 32), 3e-15 .. 8e-15;
    seeds whose movement was above 1e-14 (up to 2.3e-14) were passed over.  Uniform_Topology(260, 0.5, 0.2, 0.1, seed=9), the
    suite's own tile-test graph, moves by 2.2e-12; (40, 0.5, seed=1) by 6.8e-15.
  * MPLS on ``bridged`` with 3 bridges: R_est moved by 1e-6 .. 8e-6 on about half the seeds tried (the three bridges alone tie the two blocks'
    gauges, and an edge crossing the hard quantile threshold changes which of them count); with 5 bridges and sigma = 0.2, 3.7e-10.
  * IRLS on band(200, 10) at sigma = 0.2: R_l1 moved by 7.9e-11; at sigma = 0.1 by 2.2e-13.  (On power_law(500) at sigma = 0.2 the
    GPU and the oracle were 1.9e-9 apart in R_l1; the smaller, quieter power_law(200) moves by 1.1e-12.)
  * The LP on hub300_mid and bridged150_60 (3e5 rows): x and y after 50 plain steps moved by 2.5e-14 and 3.0e-14; on graphs of 100 and
    80 nodes by 5.5e-15 and 3.3e-15.
  * The refinement on the outlier-free hubs stops after 1 step (GCW's start is already within the threshold): its two hub shapes keep
    q = 0.3, sigma = 0.2 (20 and 25 steps), which the refinement oracle tolerates (1.7e-13)."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import refine_oracle
from oracle.cemp_oracle import cemp_oracle, cemp_oracle_batched
from oracle.spectral_oracle import gcw_oracle, rotation_alignment, spectral_oracle
from tests import graph_shapes as G
from tests import lp_oracle as LPO
from tests.graph_shapes import SHAPES, model, noisy_truth, shapes_for, ulp_perturbed
from tests.irls_oracle import irls_oracle
from tests.mpls_oracle import mpls_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1                                         # cycle-sampling key of every CEMP / MPLS case
NSAMPLE = 50                                     # Demo/compare_algorithms.m:28
NSAMPLES_EDGE = (64, 65, 256, 257, 300)          # cemp.hip:238/292/308 on one small hub graph


def demo_params():
    """Demo/compare_algorithms.m:26-36 (tests/test_gpu_mpls.py: demo_params)."""
    cemp = dict(max_iter=6, reweighting=[2.0 ** k for k in range(6)], nsample=NSAMPLE, seed=SEED)
    mpls = dict(stop_threshold=1e-3, max_iter=100, reweighting=cemp["reweighting"][-1], thresholding=[0.95, 0.9, 0.85, 0.8],
                cycle_info_ratio=1.0 / (np.arange(1, 101) + 1))
    return cemp, mpls


# ---- thresholds, out of the sources -----------------------------------------------------------------------------------------------
def _src(*parts):
    with open(os.path.join(ROOT, "desc_amd", "csrc", *parts)) as f:
        return f.read()


def _one(pattern, text, what):
    found = re.findall(pattern, text)                # the plain and the tile kernel of CEMP's rounds repeat a branch: they must agree
    assert found and len(set(found)) == 1, (what, pattern, found)
    return found[0]


@functools.lru_cache(maxsize=None)
def thresholds():
    cemp, sd, sp, mst = _src("cemp.hip"), _src("structure_device.hip"), _src("spectral.hip"), _src("mst.hip")
    K = dict(
        CEMP_MAXB=int(_one(r"constexpr int CEMP_MAXB = (\d+);", cemp, "nodes per band")),
        TILE_LDS=1024 * int(_one(r"\(size_t\)max_deg \* sizeof\(double\) <= (\d+) \* 1024", cemp, "tiles: one row in the LDS")),
        S0_BYTES=8 * int(_one(r"lds0 = \(size_t\)max_deg \* (\d+) \* sizeof\(double\)", cemp, "staged S0: bytes per slot")),
        S0_MAX=1024 * int(_one(r"tiles && lds0 <= (\d+) \* 1024", cemp, "staged S0: largest LDS")),
        S0_OPTIN=1024 * int(_one(r"if \(lds0 > (\d+) \* 1024\) DESC_HIP\(hipFuncSetAttribute", cemp, "staged S0: opt-in above")),
        BAND_LDS=1024 * int(_one(r"\((\d+) \* 1024 / 8\) / std::max\(max_deg, 1\)", cemp, "band rows per tile")),
        NS_LANE=int(_one(r"if \(nsample <= (\d+)\) \{", cemp, "one sample per lane")),
        NS_REG=64 * int(_one(r"if \(nsample <= (\d+) \* 64\) \{", cemp, "weights in registers")),
        MAX_CODEG_LDS=int(_one(r"constexpr int MAX_CODEG_LDS = (\d+);", sd, "device builder")),
        SAMPLER_X=int(_one(r"max_codeg > (\d+) \* MAX_CODEG_LDS", sd, "device sampler")),
        WIDE=int(_one(r"wide_rows = 2 \* m >= (\d+) \* n", sp, "workgroup per row")),
        BAND_ROW_CAP=int(_one(r"constexpr int BAND_ROW_CAP = (\d+);", _src("node_plan.h"), "band rows of the sweep")),
        MST_ROUNDS=int(_one(r"max_rounds = log2n \+ (\d+), jumps = log2n \+ \d+;", mst, "Boruvka rounds")),
        MST_JUMPS=int(_one(r"max_rounds = log2n \+ \d+, jumps = log2n \+ (\d+);", mst, "pointer jumps")),
    )
    assert "lo = -sigma; tight_ok = false;" in sp                    # spectral.hip:555: the fallback the bipartite shapes are there for
    assert "if (v < n && v > 0)" in _src("laa.hip")                   # laa.hip:109: node 1 is the grounded one
    return K


@functools.lru_cache(maxsize=None)
def facts(name):
    mo = model(name)
    Ind = mo.Ind
    n, m = mo.n, Ind.shape[0]
    deg, cod = G.degrees(Ind), G.codegrees(Ind)
    pos = cod > 0
    nopos = np.flatnonzero(~pos)
    return dict(n=n, m=m, deg=deg, max_deg=int(deg.max()), min_deg=int(deg.min()), max_codeg=int(cod.max()), m_pos=int(pos.sum()),
                inside=bool(pos.any() and ((nopos > np.flatnonzero(pos)[0]) & (nopos < np.flatnonzero(pos)[-1])).any()), bipartite=G.is_bipartite(Ind),
                hubs=[int(v) + 1 for v in np.flatnonzero(deg == n - 1)], bandwidth=int((Ind[:, 1] - Ind[:, 0]).max()),
                connected=bool((G.bfs_levels(Ind) >= 0).all()))


def _tiles(f, K):
    """cemp.hip:368 (and :345: the packed positions come from the device sampler)."""
    return f["m_pos"] > 0 and 8 * f["max_deg"] <= K["TILE_LDS"] and f["max_codeg"] <= K["SAMPLER_X"] * K["MAX_CODEG_LDS"]


def _bi(f, K):
    """cemp.hip:399."""
    return max(1, min(K["CEMP_MAXB"], (K["BAND_LDS"] // 8) // max(f["max_deg"], 1)))


# side -> (where the branch is, predicate on the facts of a shape)
SIDES = {
    # cemp.hip:386-393: the staged S0 kernel keeps 80 max_deg bytes in the LDS
    "s0_staged_default": ("cemp.hip:387", lambda f, K: _tiles(f, K) and K["S0_BYTES"] * f["max_deg"] <= K["S0_OPTIN"]),
    "s0_staged_optin": ("cemp.hip:391", lambda f, K: _tiles(f, K) and K["S0_OPTIN"] < K["S0_BYTES"] * f["max_deg"] <= K["S0_MAX"]),
    "s0_plain_over_lds": ("cemp.hip:394", lambda f, K: _tiles(f, K) and K["S0_BYTES"] * f["max_deg"] > K["S0_MAX"]),
    "s0_plain_tiles_off": ("cemp.hip:394", lambda f, K: f["m_pos"] > 0 and not _tiles(f, K)),
    # cemp.hip:399 / :368: nodes per band, tiles at all
    "bi_full": ("cemp.hip:399", lambda f, K: _tiles(f, K) and _bi(f, K) == K["CEMP_MAXB"]),
    "bi_partial": ("cemp.hip:399", lambda f, K: _tiles(f, K) and 1 < _bi(f, K) < K["CEMP_MAXB"]),
    "bi_one": ("cemp.hip:399", lambda f, K: _tiles(f, K) and 8 * f["max_deg"] > K["BAND_LDS"] // 2),
    "tiles_off_by_lds": ("cemp.hip:368", lambda f, K: 8 * f["max_deg"] > K["TILE_LDS"]),
    # cemp.hip:222-235: where the long row lies; tiles that hold no edge (with 32-node j-blocks)
    "hub_row_first": ("cemp.hip:225", lambda f, K: f["hubs"] == [1]),
    "hub_row_middle": ("cemp.hip:225", lambda f, K: len(f["hubs"]) == 1 and f["n"] // 4 < f["hubs"][0] < 3 * f["n"] // 4),
    "hub_row_last": ("cemp.hip:230", lambda f, K: f["hubs"] == [f["n"]]),
    "empty_tiles": ("cemp.hip:235", lambda f, K: _tiles(f, K) and f["bandwidth"] + 32 + K["CEMP_MAXB"] < f["n"]),
    # structure_device.hip:667 -> cemp.hip:348-362, structure_device.hip:534
    "host_sampler": ("structure_device.hip:667", lambda f, K: f["max_codeg"] > K["SAMPLER_X"] * K["MAX_CODEG_LDS"]),
    "device_sampler": ("structure_device.hip:667", lambda f, K: 0 < f["max_codeg"] <= K["SAMPLER_X"] * K["MAX_CODEG_LDS"]),
    "device_builder_refuses": ("structure_device.hip:534", lambda f, K: f["max_codeg"] > K["MAX_CODEG_LDS"]),
    "device_builder_builds": ("structure_device.hip:534", lambda f, K: 0 < f["max_codeg"] <= K["MAX_CODEG_LDS"]),
    # cemp.hip:405, mpls.hip: the map edge -> index among the edges with cycles
    "every_edge_has_cycles": ("cemp.hip:405", lambda f, K: f["m_pos"] == f["m"]),
    "no_cycle_edges_inside": ("cemp.hip:405", lambda f, K: 0 < f["m_pos"] < f["m"] and f["inside"]),
    "no_edge_has_cycles": ("cemp.hip:380", lambda f, K: f["m_pos"] == 0),
    # spectral.hip:524: a workgroup per row from an average of 192 slots, a wave per row below
    "wave_per_row_long_row": ("spectral.hip:524", lambda f, K: 2 * f["m"] < K["WIDE"] * f["n"] and f["max_deg"] >= 512),
    "wg_per_row_short_row": ("spectral.hip:524", lambda f, K: 2 * f["m"] >= K["WIDE"] * f["n"] and f["min_deg"] <= 3),
    # spectral.hip:554-558: lambda_min = -lambda_max exactly
    "bipartite": ("spectral.hip:555", lambda f, K: f["bipartite"]),
    "not_bipartite": ("spectral.hip:556", lambda f, K: not f["bipartite"]),
    # laa.hip:80-121: 16 lanes per row, node 1 grounded
    "hub_is_grounded_node": ("laa.hip:109", lambda f, K: f["deg"][0] == f["n"] - 1 and f["deg"][0] >= 8 * 16),
    "hub_is_last_node": ("laa.hip:111", lambda f, K: f["deg"][-1] == f["n"] - 1 and f["deg"][0] < 64),
    "long_row": ("laa.hip:88", lambda f, K: f["max_deg"] >= 16 * 4 and f["max_deg"] >= 8 * np.median(f["deg"])),
    "uniform_narrow_rows": ("laa.hip:88", lambda f, K: f["max_deg"] <= 2 * 16 and f["max_deg"] <= 2 * f["min_deg"]),
    "largest_component_without_node_1": ("irls.hip", lambda f, K: not f["connected"]),
    # pgd_layout.hip setup_node (band_ok), node_plan.cpp: band rows up to BAND_ROW_CAP doubles
    "one_row_far_longer": ("pgd_layout.hip setup_node", lambda f, K: 20 * np.median(f["deg"]) <= f["max_deg"] <= K["BAND_ROW_CAP"]),
}


def test_thresholds_are_the_ones_the_shapes_were_sized_for():
    """The figures the shapes were sized for: max_deg 819 / 1920 / 2048 / 8192, codegree 1024 / 4096, 2 m >= 192 n.  Pinned on purpose,
    next to the predicates: a retuned constant fails here even where every shape still lies on its side, so that whoever retunes it
    looks at the table once (a shape 1 below an old threshold may sit far from the new one) and then edits these numbers."""
    K = thresholds()
    assert K["S0_OPTIN"] // K["S0_BYTES"] == 819 and K["S0_MAX"] // K["S0_BYTES"] == 1920
    assert (K["BAND_LDS"] // 8) // 2 == 2048 and K["TILE_LDS"] // 8 == 8192 and K["CEMP_MAXB"] == 16
    assert K["MAX_CODEG_LDS"] == 1024 and K["SAMPLER_X"] * K["MAX_CODEG_LDS"] == 4096
    assert K["WIDE"] == 192 and K["NS_LANE"] == 64 and K["NS_REG"] == 256
    assert K["BAND_ROW_CAP"] == 19200
    assert (K["MST_ROUNDS"], K["MST_JUMPS"]) == (2, 1)


def test_every_side_of_every_branch_is_claimed():
    claimed = {s for _, sides, _ in SHAPES.values() for s in sides}
    assert claimed == set(SIDES), (sorted(set(SIDES) - claimed), sorted(claimed - set(SIDES)))
    K = thresholds()
    lo, hi = K["NS_LANE"], K["NS_REG"]
    assert NSAMPLE <= lo and {lo, lo + 1, hi, hi + 1} <= set(NSAMPLES_EDGE) and max(NSAMPLES_EDGE) > hi + 1
    # every CEMP LDS class is run against the oracle, with the hub first, in the middle and last
    cemp = {s for k in shapes_for("cemp") for s in SHAPES[k][1]}
    assert {"s0_staged_default", "s0_staged_optin", "s0_plain_over_lds", "s0_plain_tiles_off", "bi_full", "bi_partial", "bi_one", "tiles_off_by_lds",
            "hub_row_first", "hub_row_middle", "hub_row_last", "host_sampler", "no_edge_has_cycles", "no_cycle_edges_inside"} <= cemp
    for use, sides in (("refine", {"hub_is_grounded_node", "hub_is_last_node", "uniform_narrow_rows", "no_cycle_edges_inside"}),
                       ("mpls", {"hub_is_grounded_node", "hub_is_last_node", "uniform_narrow_rows", "no_cycle_edges_inside"}),
                       ("spectral", {"wave_per_row_long_row", "wg_per_row_short_row", "bipartite", "not_bipartite"}),
                       ("gcw", {"wave_per_row_long_row", "wg_per_row_short_row", "bipartite"}),
                       ("irls", {"hub_is_grounded_node", "long_row", "uniform_narrow_rows", "largest_component_without_node_1"}),
                       ("pgd", {"one_row_far_longer"}), ("pgd_fallback", {"device_builder_refuses"})):
        got = {s for k in shapes_for(use) for s in SHAPES[k][1]}
        assert sides <= got, (use, sorted(sides - got))


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_lies_on_its_sides(name):
    f, K = facts(name), thresholds()
    print(name, {k: v for k, v in f.items() if k != "deg"})
    for side in SHAPES[name][1]:
        assert SIDES[side][1](f, K), (name, side, SIDES[side][0])
    mo = model(name)
    Ind = mo.Ind
    assert np.array_equal(Ind, Ind[np.lexsort((Ind[:, 1], Ind[:, 0]))]) and (Ind[:, 0] < Ind[:, 1]).all() and Ind.min() == 1
    assert len(np.unique(Ind, axis=0)) == f["m"] < 100_000 and f["n"] <= 8300
    assert f["min_deg"] >= 1                                                   # no isolated node id
    assert f["connected"] == (name != "two_components")
    if name == "two_components":
        lv = G.bfs_levels(Ind, 1)
        assert 2 * int((lv >= 0).sum()) < f["n"]                                # node 1 lies in the smaller piece
    if hasattr(mo, "bridge"):                                                  # the bridges, and only they, lie on no 3-cycle
        assert mo.bridge.sum() in (3, 5) and np.array_equal(G.codegrees(Ind) == 0, mo.bridge)


# ---- MST: the depth of the hook chains --------------------------------------------------------------------------------------------
MST_N = (4096, 4097, 5000)
MST_KINDS = ("increasing", "decreasing", "alternating", "equal")


def mst_weights(kind, m):
    e = np.arange(m)
    return {"increasing": e / m, "decreasing": 1.0 - e / m, "alternating": 0.5 * (e % 2), "equal": np.full(m, 0.25)}[kind]


def test_mst_cases_reach_deep_hook_chains():
    """mst.hip:124-138.  On the path with increasing weights every node's lightest edge leads to its predecessor: the first round's
    hook chain is n - 1 deep, and only ceil(log2 n) + 1 pointer jumps flatten it.  On both sides of n = 2^12."""
    K = thresholds()
    for n in MST_N:
        Ind = G.band(n, 1, seed=3).Ind
        jumps = int(np.ceil(np.log2(n))) + K["MST_JUMPS"]
        depth = {kind: G.first_round_chain_depth(Ind, mst_weights(kind, n - 1)) for kind in MST_KINDS}
        print(n, depth, "jumps", jumps)
        assert depth["increasing"] == n - 1 and depth["decreasing"] == n - 2 and depth["equal"] == n - 1 and depth["alternating"] <= 2
        need = int(np.ceil(np.log2(depth["increasing"])))                        # jumps that halve a chain of this depth to nothing
        assert jumps - 2 <= need <= jumps, (need, jumps)
    assert MST_N[0] == 2 ** 12 and MST_N[1] == 2 ** 12 + 1
    for hub_id in (1, 4097):
        Ind = G.star(4097, hub_id, seed=4).Ind
        assert G.first_round_chain_depth(Ind, mst_weights("increasing", 4096)) <= 2


def test_mst_propagation_order():
    """Along a path of 5000 rotations, R_k by the tree's breadth-first products (tests/mpls_oracle.py: propagate) and by accumulating
    the transposed product from the other side: what two multiplication orders leave between them (8.3e-15 at n = 5000, 9.9e-15 at
    4096) is 1/100 of the 1e-12 the GPU test applies, so the device may multiply in either order."""
    from tests.mpls_oracle import propagate
    for n in (MST_N[0], MST_N[-1]):
        mo = G.band(n, 1, seed=3)
        R = propagate(mo.Ind, mo.RijMat, np.arange(n - 1))
        acc, other = np.eye(3), [np.eye(3)]
        for e in range(n - 1):
            acc = acc @ mo.RijMat[:, :, e]
            other.append(acc.T)
        d = float(np.abs(np.transpose(np.array(other), (1, 2, 0)) - R).max())
        print("path of %d: two multiplication orders differ by %.2e" % (n, d))
        assert d <= 1e-12 / 100


# ---- oracle qualification --------------------------------------------------------------------------------------------------------
def aligned_diff(R, R_ref):
    return float(np.abs(rotation_alignment(R, R_ref)[0] - R_ref).max())


@functools.lru_cache(maxsize=None)
def _inputs(name, perturbed):
    mo = model(name)
    S = noisy_truth(mo, SEED)
    if perturbed:
        return mo.Ind, ulp_perturbed(mo.RijMat, 101), ulp_perturbed(S, 102)
    return mo.Ind, mo.RijMat, S


@functools.lru_cache(maxsize=None)
def run_oracle(name, which, perturbed=False):
    """One oracle on one shape.  R_init of the refinement is an input of the comparison (the unperturbed GCW oracle's), as in
    tests/test_gpu_refine.py."""
    Ind, Rij, S = _inputs(name, perturbed)
    if which == "cemp":
        return (cemp_oracle_batched(Ind, Rij, 6, 2.0 ** np.arange(6), NSAMPLE, seed=SEED),)
    if which.startswith("cemp_ns"):                                             # the unbatched restatement, as the GPU test uses it
        return (cemp_oracle(Ind, Rij, 6, 2.0 ** np.arange(6), int(which[7:]), seed=SEED),)
    if which == "pgd":                                                          # the C oracle: structure seed 0, 20 constant steps
        from oracle import oracle as O
        from desc_amd.algorithms import marshal_edges
        O.build(); O.lib()
        nn, ii, jj, rij, _ = marshal_edges(Ind, Rij)
        st = O.build_structure(nn, ii, jj, seed=0)
        out = O.pgd_run(st, O.cycle_d(ii, jj, rij.reshape(-1, 9), st), 100 if name in shapes_for("gcw") else 20, lr=0.01)
        return (out["S_vec"],)
    if which == "lp":                                                           # 50 plain PDHG steps on the restated LP
        K, b, pos, k, ns = LPO.build_lp(Ind, Rij, SEED)
        tau, sigma = LPO.step_sizes(K)
        x, y = LPO.pdhg_plain(K, b, tau, sigma, 50)
        return (np.concatenate([x, y]),)
    if which == "spectral":
        return (spectral_oracle(Ind, Rij),)
    if which == "gcw":
        return (gcw_oracle(Ind, Rij, S),)
    if which == "refine":
        R_init = run_oracle(name, "gcw")[0]
        trace = []
        inner = refine_oracle.Weighted_LAA

        def recording(I, Q, QQ, Amatrix, Weights):
            out = inner(I, Q, QQ, Amatrix, Weights)
            trace.append((Weights.copy(), out[2].copy()))
            return out
        refine_oracle.Weighted_LAA = recording
        try:
            R, iters, score = refine_oracle.desc_refine_oracle(Ind, Rij, S, R_init)
        finally:
            refine_oracle.Weighted_LAA = inner
        return R, iters, score, trace
    if which == "mpls":
        cemp, mpls = demo_params()
        tree_S = None if not perturbed else run_oracle(name, "mpls")[3]          # the tree is an input of the comparison (mpls_oracle)
        r = mpls_oracle(Ind, Rij, cemp, mpls, seed=SEED, svec_for_tree=tree_S)
        return r["R_est"], r["iters"], r["score"], r["SVec"], r["R_init"]
    if which in ("irls_GM", "irls_L12"):
        R, R_l1, tr = irls_oracle(Rij, Ind, which[5:])
        return np.nan_to_num(R), (tr["l1_iters"], tr["irls_iters"], tr["steps"]), 0.0, np.nan_to_num(R_l1)
    raise KeyError(which)


# use -> tolerance of tests/test_gpu_graph_shapes.py (and where it comes from)
TOL = dict(cemp=1e-12,            # tests/test_gpu_cemp.py
           spectral=1e-8,         # tests/test_gpu_spectral.py, after alignment
           gcw=1e-8,
           refine=1e-7,           # tests/test_gpu_refine.py
           mpls=1e-7,             # tests/test_gpu_mpls.py: check_against_oracle (R_init 1e-10, SVec 1e-12, score 1e-9)
           irls_GM=1e-7,          # tests/test_gpu_irls.py: check (R_l1 1e-9)
           irls_L12=1e-7,
           pgd=1e-10,             # tests/test_gpu_sweep_instances.py
           lp=1e-12)              # tests/test_gpu_lp.py: pdhg_plain
TOL.update({"cemp_ns%d" % ns: 1e-12 for ns in NSAMPLES_EDGE})

QUALIFY = [(name, use) for use in ("cemp", "spectral", "gcw", "refine", "mpls") for name in shapes_for(use)]
QUALIFY += [(name, use) for use in ("irls_GM", "irls_L12") for name in shapes_for("irls")]
QUALIFY += [(name, "cemp") for name in shapes_for("mpls") if name not in shapes_for("cemp")]      # SVec at 1e-12 there too
QUALIFY += [(name, "cemp_ns%d" % ns) for name in shapes_for("cemp_nsample") for ns in NSAMPLES_EDGE]
QUALIFY += [(name, "pgd") for name in shapes_for("pgd")] + [(name, "lp") for name in shapes_for("lp")]


@pytest.mark.parametrize("name,use", QUALIFY, ids=["%s-%s" % (u, n) for n, u in QUALIFY])
def test_oracle_moves_less_than_a_hundredth_of_the_tolerance(name, use):
    a, b = run_oracle(name, use), run_oracle(name, use, True)
    if use in ("spectral", "gcw"):
        move = aligned_diff(b[0], a[0])
    else:
        move = float(np.abs(b[0] - a[0]).max())
    print("%s %s: oracle movement under +-1 ulp of its inputs %.2e (tolerance %.0e)" % (use, name, move, TOL[use]))
    assert move <= TOL[use] / 100, (name, use, move)
    if use.startswith("irls"):
        move1 = float(np.abs(b[3] - a[3]).max())
        print("   R_l1 moves %.2e (tolerance 1e-09); iterations %s" % (move1, a[1]))
        assert move1 <= 1e-9 / 100 and a[1] == b[1]
    if use in ("refine", "mpls"):
        print("   steps %d / %d, score %.6e / %.6e" % (a[1], b[1], a[2], b[2]))
        assert a[1] == b[1] and a[1] >= 4                                       # the quantile threshold really moves; the count is stable
        assert abs(a[2] - b[2]) <= 1e-9 / 100
    if use == "mpls":
        assert np.abs(a[3] - b[3]).max() <= 1e-12 / 100 and np.abs(a[4] - b[4]).max() <= 1e-10 / 100


PCG_SHAPES = sorted(set(shapes_for("refine")) | set(shapes_for("mpls")) | set(shapes_for("irls")))


@functools.lru_cache(maxsize=None)
def _five_refinement_steps(name):
    """(Ind, trace) of the refinement oracle on the shape's largest component, run for exactly 5 steps (stop_threshold 0): step 1 has the
    quantile 1.0, step 5 is the first with 0.8 (DESC.m:276, :297)."""
    mo = model(name)
    lv = G.bfs_levels(mo.Ind, 1)
    keep = np.ones(mo.n, dtype=bool) if (lv >= 0).all() else (lv < 0 if 2 * (lv >= 0).sum() < lv.size else lv >= 0)
    e = keep[mo.Ind[:, 0] - 1] & keep[mo.Ind[:, 1] - 1]
    Ind, Rij, S = np.cumsum(keep)[mo.Ind[e] - 1], mo.RijMat[:, :, e], noisy_truth(mo, SEED)[e]
    trace = []
    inner = refine_oracle.Weighted_LAA

    def recording(I, Q, QQ, Amatrix, Weights):
        out = inner(I, Q, QQ, Amatrix, Weights)
        trace.append((Weights.copy(), out[2].copy()))
        return out
    refine_oracle.Weighted_LAA = recording
    try:
        refine_oracle.desc_refine_oracle(Ind, Rij, S, gcw_oracle(Ind, Rij, S), stop_threshold=0.0, maxIters=6)
    finally:
        refine_oracle.Weighted_LAA = inner
    assert len(trace) == 5
    return Ind, trace


@pytest.mark.parametrize("name", PCG_SHAPES)
def test_jacobi_pcg_finishes_within_half_the_cap(name):
    """Weights as DESC.m:279-282 leaves them (truncated to 1e-4 above the quantile, up to 1e4 below) at the first step of the refinement
    oracle and at its fifth, the first whose quantile is 0.8; right-hand side A' W^2 B of that step.  On every shape the refinement,
    MPLS or IRLS run on (two_components: its largest component)."""
    Ind, trace = _five_refinement_steps(name)
    steps = [trace[0], trace[4]]
    n = int(Ind.max())
    cap = min(20000, 20 * n + 200)
    for W, B in steps:
        w2B = (W ** 2)[:, None] * B
        rhs = np.zeros((n, 3))
        np.add.at(rhs, Ind[:, 1] - 1, w2B); np.add.at(rhs, Ind[:, 0] - 1, -w2B)
        x, iters = G.jacobi_pcg(Ind, W, rhs)
        print("%s: Jacobi-PCG %d iterations (cap %d), weights %.1e .. %.1e" % (name, iters, cap, W.min(), W.max()))
        assert 2 * iters <= cap, (name, iters, cap)
        if n <= 600:                                                            # the restated solver solves the grounded system
            A = refine_oracle.Build_Amatrix(Ind.T)
            ref = np.linalg.lstsq(W[:, None] * A, W[:, None] * B, rcond=None)[0]
            assert np.abs(x[1:] - ref).max() <= 1e-8 * max(1.0, np.abs(ref).max())

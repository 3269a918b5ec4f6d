"""The graph kernels on hub, band, star, bipartite, bridged and power-law graphs (tests/graph_shapes.py), each against the plain
restatement of the same operation.  Every graph the rest of the suite feeds to the library is Erdos-Renyi: degrees within a few
percent of n p, one component, diameter 2-3, a large spectral gap, never bipartite, every edge on a 3-cycle.  The code next to the
sweep chooses its paths from the shape of the graph; tests/test_graph_shapes.py (CPU) names the branches, reads their thresholds out
of the sources, and checks that the shapes lie where they are meant to and that the oracles are well-conditioned on them.

Tolerances are the project's existing ones, unchanged:
  CEMP SVec 1e-12 (tests/test_gpu_cemp.py); Spectral / GCW 1e-8 after alignment (tests/test_gpu_spectral.py); refinement and MPLS
  R_est 1e-7, R_init 1e-10, score 1e-9, equal iteration counts (tests/test_gpu_refine.py, tests/test_gpu_mpls.py: check_against_oracle);
  MST tree array_equal to Kruskal, propagation 1e-12 (tests/test_gpu_mpls.py); PGD 1e-10 with assert_structure_equal
  (tests/test_gpu_sweep_instances.py); IRLS 1e-9 / 1e-7 with equal step counts (tests/test_gpu_irls.py: check); LP through
  pdhg_plain at 1e-12 and the certificates (tests/test_gpu_lp.py).

Oracle sensitivities and PCG iteration counts that justify applying them to these graphs: tests/test_graph_shapes.py, QUALIFIED."""
import numpy as np
import pytest

from desc_amd import CEMP, DESC_PGD, GCW, MST, ConstantStepSize, Spectral, _lib, linprog_sij
from desc_amd.algorithms import marshal_edges
from oracle.cemp_oracle import cemp_oracle, cemp_oracle_batched
from oracle.refine_oracle import desc_refine_oracle
from oracle.spectral_oracle import gcw_oracle, rotation_alignment, spectral_oracle
from tests import graph_shapes as G
from tests import lp_oracle as LPO
from tests.graph_shapes import model, noisy_truth, shapes_for
from tests.helpers import assert_structure_equal, c_params, emulate_sharded
from tests.mpls_oracle import kruskal, propagate
from tests.test_gpu_irls import check as irls_check
from tests.test_gpu_mpls import check_against_oracle
from tests.test_graph_shapes import MST_KINDS, MST_N, NSAMPLE, NSAMPLES_EDGE, SEED, demo_params, mst_weights

pytestmark = pytest.mark.gpu

BETA = 2.0 ** np.arange(6)                          # Demo/compare_algorithms.m:26-28
_ref = {}


def cemp_params(nsample=NSAMPLE):
    return dict(max_iter=6, reweighting=BETA, nsample=nsample, seed=SEED)


def cemp_reference(name):
    if name not in _ref:
        mo = model(name)
        _ref[name] = cemp_oracle_batched(mo.Ind, mo.RijMat, 6, BETA, NSAMPLE, seed=SEED)
    return _ref[name]


def aligned_diff(R, R_ref):
    return float(np.abs(rotation_alignment(R, R_ref)[0] - R_ref).max())


def so3_defect(R):
    Rm = np.transpose(R, (2, 0, 1))
    return max(float(np.abs(Rm @ np.transpose(Rm, (0, 2, 1)) - np.eye(3)).max()), float(np.abs(np.linalg.det(Rm) - 1).max()))


# ---- CEMP -----------------------------------------------------------------------------------------------------------------------
CEMP_HUBS = ["hub300_mid", "hub900_first", "hub2000_mid", "hub2100_last", "hub8300_mid"]


@pytest.mark.parametrize("name", CEMP_HUBS)
def test_cemp_hub_matches_oracle_in_every_lds_class(name, monkeypatch):
    """cemp.hip:386-393, :399, :368: max_deg <= 819 / 820..1920 / 1921..2048 / 2049..8192 / > 8192, the hub first, in the middle and
    last.  Then the cross-checks of tests/test_gpu_cemp.py, bit for bit: tiles off, the staged layout off, and j-blocks of 32 and 50
    nodes, which the hub's row crosses dozens of times (cemp.hip:222-235)."""
    mo = model(name)
    S = CEMP(mo.Ind, mo.RijMat, cemp_params())
    d = float(np.abs(S - cemp_reference(name)).max())
    print("%s: max|SVec - oracle| %.3e" % (name, d))
    assert d < 1e-12
    for env in (dict(DESC_DEBUG_CEMP_TILES="0"), dict(DESC_DEBUG_STAGED_LAYOUT="0"), dict(DESC_DEBUG_CEMP_JB="32"), dict(DESC_DEBUG_CEMP_JB="50")):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            assert np.array_equal(CEMP(mo.Ind, mo.RijMat, cemp_params()), S), env


def test_cemp_two_adjacent_hubs_take_the_host_sampler():
    """structure_device.hip:667 -> cemp.hip:348-362: the edge (1, 2) has n - 2 > 4096 common neighbours, the device sampler answers
    DESC_ERR_TOO_LARGE and the host sampler's cycles feed the plain rounds (no packed positions: no tiles)."""
    mo = model("hubs4100_adjacent")
    S = CEMP(mo.Ind, mo.RijMat, cemp_params())
    d = float(np.abs(S - cemp_reference("hubs4100_adjacent")).max())
    print("hubs4100_adjacent: max|SVec - oracle| %.3e" % d)
    assert d < 1e-12


def test_linprog_sij_refuses_a_codegree_above_the_sampler_budget():
    """cemp.hip:349: nsample = 0 (linprog_sij's default: the rule of linprog_sij.m:43) is the device sampler's business, so a codegree
    above 4096 is DESC_ERR_TOO_LARGE with the sampler's message (include/desc_amd.h: desc_lp_sij_run)."""
    mo = model("hubs4100_adjacent")
    with pytest.raises(_lib.DescError, match="common neighbours") as ei:
        linprog_sij(mo.Ind, mo.RijMat, dict(seed=SEED, max_iter=1))
    assert ei.value.code == _lib.ERR_TOO_LARGE


def test_linprog_sij_with_explicit_nsample_takes_the_host_sampler():
    """With nsample given the host sampler serves the same graph: the variables and the sampled third nodes of tests/lp_oracle.py, and
    one plain step equal to pdhg_plain at 1e-12."""
    mo = model("hubs4100_adjacent")
    K, b, pos, k, ns = LPO.build_lp(mo.Ind, mo.RijMat, SEED, nsample=37)
    _, S, info = linprog_sij(mo.Ind, mo.RijMat, dict(seed=SEED, tol=0.0, restart=0, max_iter=1, return_dual=True, nsample=37), return_info=True)
    assert info["lp"]["nsample"] == ns == 37 and info["lp"]["m_pos"] == pos.size == mo.Ind.shape[0]
    assert np.array_equal(info["pos_edges"], pos) and np.array_equal(info["k"], k)
    tau, sigma = LPO.step_sizes(K)
    x, y = LPO.pdhg_plain(K, b, tau, sigma, 1)
    assert np.abs(S[pos] - x).max() <= 1e-12 and np.abs(info["y"].reshape(-1) - y).max() <= 1e-12


@pytest.mark.parametrize("name", ["star200_mid", "bipartite60_90"])
def test_cemp_without_any_cycle_is_all_ones(name):
    """cemp.hip:380-384: m_pos = 0 (CEMP.m:103)."""
    mo = model(name)
    assert np.array_equal(CEMP(mo.Ind, mo.RijMat, cemp_params()), np.ones(mo.Ind.shape[0]))


@pytest.mark.parametrize("env", [{}, dict(DESC_DEBUG_CEMP_TILES="0"), dict(DESC_DEBUG_CEMP_JB="32")], ids=["default", "plain", "jb32"])
@pytest.mark.parametrize("name", ["bridged150_60", "band200_10"])
def test_cemp_bridges_and_bands(name, env, monkeypatch):
    """cemp.hip:405: the bridges lie on no 3-cycle and sit inside the edge list -- exactly they stay 1.0.  The band graph's tiles
    far from the diagonal hold no edge (cemp.hip:235) once the j-blocks are 32 nodes."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mo = model(name)
    S = CEMP(mo.Ind, mo.RijMat, cemp_params())
    if name == "bridged150_60":
        assert np.array_equal(S == 1.0, mo.bridge)
    d = float(np.abs(S - cemp_reference(name)).max())
    print("%s %s: max|SVec - oracle| %.3e" % (name, env, d))
    assert d < 1e-12


@pytest.mark.parametrize("nsample", NSAMPLES_EDGE)
def test_cemp_samples_per_edge_at_the_kernel_edges(nsample, monkeypatch):
    """cemp.hip:238/292/308: one sample per lane up to 64, weights in registers up to 256, two passes above; tile and plain kernel."""
    mo = model(shapes_for("cemp_nsample")[0])
    ref = cemp_oracle(mo.Ind, mo.RijMat, 6, BETA, nsample, seed=SEED)
    for tiles in ("1", "0"):
        monkeypatch.setenv("DESC_DEBUG_CEMP_TILES", tiles)
        S = CEMP(mo.Ind, mo.RijMat, cemp_params(nsample))
        d = float(np.abs(S - ref).max())
        print("nsample %d tiles %s: max|SVec - oracle| %.3e" % (nsample, tiles, d))
        assert d < 1e-12


# ---- MST ------------------------------------------------------------------------------------------------------------------------
def _mst_case(mo, S):
    R, info = MST(mo.Ind, mo.RijMat, S, return_info=True)
    tree = kruskal(mo.Ind, S)
    assert np.array_equal(info["tree_edges"], tree)
    d = float(np.abs(R - propagate(mo.Ind, mo.RijMat, tree)).max())
    assert d < 1e-12, d                  # two multiplication orders along such a path: tests/test_graph_shapes.py::test_mst_propagation_order


@pytest.mark.parametrize("kind", MST_KINDS)
@pytest.mark.parametrize("n", MST_N)
def test_mst_on_a_path(n, kind):
    """mst.hip:124-138: with increasing weights the first round's hook chain is n - 1 deep (tests/test_graph_shapes.py)."""
    mo = G.band(n, 1, seed=3)
    _mst_case(mo, mst_weights(kind, n - 1))


@pytest.mark.parametrize("kind", MST_KINDS)
@pytest.mark.parametrize("hub_id", [1, 4097])
def test_mst_on_a_star(hub_id, kind):
    """One row of n - 1 slots under the wave-per-row minimum (mst.hip:40-63), as the root of the tree and as its last node."""
    mo = G.star(4097, hub_id, seed=4)
    _mst_case(mo, mst_weights(kind, 4096))


# ---- MPLS -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", shapes_for("mpls"))
def test_mpls_matches_oracle(name):
    mo = model(name)
    cemp, mpls = demo_params()
    R_est, R_init, info, ref = check_against_oracle(mo.Ind, mo.RijMat, cemp, mpls, SEED)
    print("%s: iters %d, cg_iters %d, cg_residual %.2e, max|R_est - oracle| %.3e" % (name, info["iters"], info["cg_iters"], info["cg_residual"],
                                                                                  np.abs(R_est - ref["R_est"]).max()))
    assert info["iters"] >= 4 and info["cg_unconverged"] == 0
    assert info["m_pos"] == int(ref["state"]["IndPosbin"].sum())
    if hasattr(mo, "bridge"):                                                    # the H step keeps the 2/3 rule on the bridges
        assert np.array_equal(~ref["state"]["IndPosbin"], mo.bridge) and np.all(info["SVec"][mo.bridge] == 1.0)


# ---- Spectral / GCW -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", shapes_for("spectral"))
def test_spectral_matches_dense_oracle(name, monkeypatch, capfd):
    """spectral.hip:524: a wave per row meets a row of 599 slots, a workgroup per row rows of 1 and 2.  spectral.hip:554-558: on a
    bipartite graph lambda_min = -lambda_max; the drift fallback must fire (its DESC_DEBUG_TIMING line), and the tight lower bound and
    the fixed scheme must agree."""
    mo = model(name)
    monkeypatch.setenv("DESC_DEBUG_TIMING", "1")
    capfd.readouterr()
    R, info = Spectral(mo.Ind, mo.RijMat, return_info=True)
    fell_back = "back to the safe lower bound" in capfd.readouterr().err
    monkeypatch.delenv("DESC_DEBUG_TIMING")
    print("%s: drift fallback of spectral.hip:559 fired: %s" % (name, fell_back))
    if "bipartite" in G.SHAPES[name][1]:         # lambda_min = -lambda_max: the block drifts to the negative end and the safe bound comes back
        assert fell_back
    R_ref = spectral_oracle(mo.Ind, mo.RijMat)
    d = aligned_diff(R, R_ref)
    print("%s: aligned max|R - oracle| %.3e, %d products, residual %.2e, eigenvalues %s" % (name, d, info["products"], info["residual"], info["eigenvalues"][:6]))
    assert info["converged"], info
    assert d < 1e-8, (d, info)
    assert so3_defect(R) < 1e-12
    if "bipartite" in G.SHAPES[name][1]:
        monkeypatch.setenv("DESC_DEBUG_SPECTRAL_TIGHT", "0")
        R0, info0 = Spectral(mo.Ind, mo.RijMat, return_info=True)
        assert info0["converged"] and aligned_diff(R0, R_ref) < 1e-8 and aligned_diff(R0, R) < 1e-8


@pytest.mark.parametrize("kind", ["pgd", "noisy_truth"])
@pytest.mark.parametrize("name", shapes_for("gcw"))
def test_gcw_matches_dense_oracle(oracle, name, kind, monkeypatch, capfd):
    """S_vec as DESC uses it (the PGD oracle's, DESC.m:263; edges without a 3-cycle keep 1) and the synthetic one of
    tests/test_gpu_spectral.py."""
    mo = model(name)
    if kind == "pgd":
        nn, ii, jj, rij, _ = marshal_edges(mo.Ind, mo.RijMat)
        st = oracle.build_structure(nn, ii, jj, seed=0)
        S = np.ones(ii.shape[0]) if st["m_pos"] == 0 else oracle.pgd_run(st, oracle.cycle_d(ii, jj, rij.reshape(-1, 9), st), 100, lr=0.01)["S_vec"]
    else:
        S = noisy_truth(mo, SEED)
    monkeypatch.setenv("DESC_DEBUG_TIMING", "1")
    capfd.readouterr()
    R, info = GCW(mo.Ind, mo.AdjMat, mo.RijMat, S, return_info=True)
    fell_back = "back to the safe lower bound" in capfd.readouterr().err
    monkeypatch.delenv("DESC_DEBUG_TIMING")
    print("%s %s: drift fallback of spectral.hip:559 fired: %s" % (name, kind, fell_back))
    R_ref = gcw_oracle(mo.Ind, mo.RijMat, S)
    d = aligned_diff(R, R_ref)
    print("%s %s: aligned max|R - oracle| %.3e, %d products, residual %.2e" % (name, kind, d, info["products"], info["residual"]))
    assert info["converged"], info
    assert d < 1e-8, (d, info)
    assert so3_defect(R) < 1e-12
    if "bipartite" in G.SHAPES[name][1]:         # the fixed scheme: on the star (spectrum {1, 0, -1}) it has to halve the degree of a pass
        monkeypatch.setenv("DESC_DEBUG_SPECTRAL_TIGHT", "0")
        R0, info0 = GCW(mo.Ind, mo.AdjMat, mo.RijMat, S, return_info=True)
        print("%s %s fixed scheme: %d products, aligned max|R - oracle| %.3e" % (name, kind, info0["products"], aligned_diff(R0, R_ref)))
        assert info0["converged"] and aligned_diff(R0, R_ref) < 1e-8
        if name.startswith("star"):
            # spectral_impl's fixed scheme takes one product per Rayleigh-Ritz and CHEB_DEG = 16 per pass: 17 iters - 16 when it
            # converges at Rayleigh-Ritz number `iters` and no pass is repeated.  A pass whose filtered block has a singular Gram
            # matrix is repeated with half the degree (8, then 4, 2), which adds that many products.
            extra = info0["products"] - (17 * info0["iters"] - 16)
            assert extra >= 8 and extra % 2 == 0, info0


# ---- refinement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", shapes_for("refine"))
def test_refinement_matches_dense_oracle(name):
    """laa.hip:80-121, :341 from the same S_vec and R_init (the GCW oracle's): the long row as the grounded node 1 and as node n, uniform
    narrow rows over a long diameter, bridges, power-law rows."""
    mo = model(name)
    S = noisy_truth(mo, SEED)
    R_init = gcw_oracle(mo.Ind, mo.RijMat, S)
    nn, ii, jj, rij, _ = marshal_edges(mo.Ind, mo.RijMat)
    R, info = _lib.refine_run(_lib.ProblemArrays(nn, ii, jj, rij), S, R_init)
    R_ref, iters_ref, score_ref = desc_refine_oracle(mo.Ind, mo.RijMat, S, R_init)
    d = float(np.abs(R - R_ref).max())
    print("%s: iters %d (oracle %d), cg_iters %d, cg_residual %.2e, max|R - oracle| %.3e" % (name, info["iters"], iters_ref, info["cg_iters"], info["cg_residual"], d))
    assert info["iters"] == iters_ref >= 4, (info, iters_ref)
    assert info["cg_unconverged"] == 0 and info["cg_residual"] <= 1e-12
    assert d < 1e-7
    assert abs(info["score"] - score_ref) < 1e-9


# ---- IRLS -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["GM", "L12"])
@pytest.mark.parametrize("name", shapes_for("irls"))
def test_irls_matches_oracle(name, mode):
    mo = model(name)
    R, info, tr = irls_check(mo.RijMat, mo.Ind, mode)
    assert info["pd_ill"] == 0 and info["pd_stuck"] == 0
    if name == "two_components":                                                  # the larger piece does not hold node 1
        assert info["comp_nodes"] == 60 and np.isnan(R[:, :, :20]).all() and not np.isnan(R[:, :, 20:]).any()


# ---- PGD sweep ------------------------------------------------------------------------------------------------------------------
PGD_ITERS = 20


def _pgd_reference(oracle, name):
    key = ("pgd", name)
    if key not in _ref:
        mo = model(name)
        nn, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
        assert perm is None
        st = oracle.build_structure(nn, ii, jj, seed=0)
        S0 = oracle.cycle_d(ii, jj, rij.reshape(-1, 9), st)
        _ref[key] = (nn, ii, jj, rij, st, S0, oracle.pgd_run(st, S0, PGD_ITERS, lr=0.01))
    return _ref[key]


@pytest.mark.parametrize("variant", ["1", "2", "3"])
@pytest.mark.parametrize("name", shapes_for("pgd"))
def test_sweep_layouts_on_a_long_row(lib, oracle, name, variant, monkeypatch):
    """pgd_layout.hip setup_node (band_ok), node_plan.cpp: one row far longer than the rest through the gather, node and band layouts on one rank."""
    monkeypatch.setenv("DESC_DEBUG_VARIANT", variant)
    nn, ii, jj, rij, st, S0, ref = _pgd_reference(oracle, name)
    prob = lib.ProblemArrays(nn, ii, jj, rij)
    dst = lib.Structure.build(prob, 30, 0, lib.BUILD_HOST, 0)
    arrays = dst.arrays()
    solver = lib.Solver(prob, dst, 0)
    try:
        s0 = solver.s0()
        out = solver.run(c_params(PGD_ITERS, lr=0.01, seed=0), want_w=True)
        last = solver.last_sweep()
    finally:
        solver.destroy(); dst.free()
    d = float(np.abs(out["S_vec"] - ref["S_vec"]).max())
    print("%s variant %s: %s, max|S - oracle| %.3e" % (name, variant, last, d))
    assert {"1": "k_sweep<", "2": "k_sweep_node<", "3": "k_sweep_band<"}[variant] in last or (variant == "1" and "k_sweep_big<" in last), last
    assert_structure_equal(arrays, st)
    assert np.abs(s0 - S0).max() <= 1e-14
    assert out["iters_run"] == ref["iters_run"]
    assert d <= 1e-10 and np.abs(out["w"] - ref["w"]).max() <= 1e-10
    assert np.allclose(out["obj"], ref["obj"], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("world", [2, 3])
def test_band_sweep_sharded_on_a_long_row(lib, oracle, world, monkeypatch):
    """The hub graph through the band sweep on 2 and 3 emulated ranks (tests/helpers.py), host structure, against the C oracle."""
    monkeypatch.setenv("DESC_DEBUG_VARIANT", "3")
    name = "hub1500_mid"
    nn, ii, jj, rij, st, S0, ref = _pgd_reference(oracle, name)
    monkeypatch.setenv("DESC_DEBUG_ROW_CAP", str(max(model(name).n, 2 * ii.shape[0] // 12)))      # ~12 bands: every rank gets a range of them
    outs, segs = emulate_sharded(lib, nn, ii, jj, rij, c_params(PGD_ITERS, lr=0.01, seed=0), world, where=lib.BUILD_HOST, nmin=30)
    assert segs[0][0] == 0 and segs[-1][1] == st["m_pos"] and segs[-1][3] == st["m_cycle"]
    assert sum(sg[1] > sg[0] for sg in segs) >= 2, segs
    for out in outs:
        assert "k_sweep_band<" in out["last_sweep"], out["last_sweep"]
        assert out["iters_run"] == ref["iters_run"]
        assert np.abs(out["S_vec"] - ref["S_vec"]).max() <= 1e-10
        assert np.allclose(out["obj"], ref["obj"], rtol=1e-12, atol=1e-9)


def test_two_adjacent_hubs_fall_back_to_the_host_builder(lib):
    """structure_device.hip:534: the edge (1, 2) has 1098 > 1024 common neighbours.  The logic of
    tests/test_gpu_fullsize.py::test_device_builder_budget_falls_back_to_the_host_builder at a thousandth of its cycles."""
    mo = model("hubs1100_adjacent")
    nn, ii, jj, rij, _ = marshal_edges(mo.Ind, mo.RijMat)
    prob = lib.ProblemArrays(nn, ii, jj, rij)
    with pytest.raises(lib.DescError) as ei:
        lib.Structure.build(prob, 30, 2, lib.BUILD_DEVICE, 0)
    assert ei.value.code == lib.ERR_TOO_LARGE
    st = lib.Structure.build(prob, 30, 2, lib.BUILD_HOST, 0)
    assert st.sizes()["m_cycle"] < 1_000_000
    solver = lib.Solver(prob, st, 0)
    st.free()
    ref = solver.run(c_params(3, lr=0.01, seed=2))
    solver.destroy()
    par = lambda: dict(iters=3, Gradient=ConstantStepSize(0.01), seed=2, verbose=False)      # noqa: E731
    S_one = DESC_PGD(mo.Ind, mo.RijMat, par())
    S_three, info = DESC_PGD(mo.Ind, mo.RijMat, par(), return_info=True)
    assert np.array_equal(S_one, ref["S_vec"]) and np.array_equal(S_three, ref["S_vec"]) and info["iters_run"] == 3
    assert ((ref["S_vec"] >= 0) & (ref["S_vec"] <= 1)).all()


# ---- LP -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", shapes_for("lp"))
def test_lp_follows_the_plain_recurrence_and_certifies(name):
    """tests/test_gpu_lp.py::test_kernels_follow_the_plain_recurrence and ::test_certificates on a hub row and on bridges."""
    mo = model(name)
    K, b, pos, k, ns = LPO.build_lp(mo.Ind, mo.RijMat, SEED)
    nopos = np.setdiff1d(np.arange(mo.Ind.shape[0]), pos)
    tau, sigma = LPO.step_sizes(K)
    for N in (1, 50):
        _, S, info = linprog_sij(mo.Ind, mo.RijMat, dict(seed=SEED, tol=0.0, restart=0, max_iter=N, return_dual=True), return_info=True)
        x, y = LPO.pdhg_plain(K, b, tau, sigma, N)
        dx, dy = np.abs(S[pos] - x).max(), np.abs(info["y"].reshape(-1) - y).max()
        print("%s N %d: max|x - x_ref| %.3e  max|y - y_ref| %.3e" % (name, N, dx, dy))
        assert info["lp"]["nsample"] == ns and np.array_equal(info["pos_edges"], pos) and np.array_equal(info["k"], k)
        assert info["lp"]["iters"] == N and info["lp"]["converged"] == 0 and info["lp"]["restarts"] == 0
        assert dx <= 1e-12 and dy <= 1e-12
        assert np.all(S[nopos] == 1.0)
    tol = 1e-5
    _, S, info = linprog_sij(mo.Ind, mo.RijMat, dict(seed=SEED, tol=tol, return_dual=True), return_info=True)
    lp = info["lp"]
    viol, P, D = LPO.certificates(K, b, S[pos], info["y"].reshape(-1))
    print("%s: iters %d restarts %d  viol %.3e  P %.12g  D %.12g" % (name, lp["iters"], lp["restarts"], viol, P, D))
    assert lp["converged"] == 1 and viol <= tol and P - D <= tol * (1 + abs(P) + abs(D))
    assert np.all(info["y"] >= 0) and np.all(S >= 0) and np.all(S <= 1) and np.all(S[nopos] == 1.0)
    if hasattr(mo, "bridge"):
        assert np.array_equal(nopos, np.flatnonzero(mo.bridge))
    for got, want in ((lp["viol"], viol), (lp["pobj"], P), (lp["dobj"], D)):
        assert abs(got - want) <= 1e-9 * abs(want) + 1e-15, (got, want)

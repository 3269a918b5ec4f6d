"""The references of tests/test_gpu_laa_maps.py checked without a GPU, on the same inputs (tests/laa_maps_cases.py): restatement (a)
(float64, the kernels' bracketing) against the 50-digit formulas (b), against oracle/refine_oracle.py's R2Q, q2R, qmul and Weighted_LAA,
against tests/irls_oracle.py's edge_log / exp_update / project, and NumPy's 'hazen' quantile; the cases are checked to reach the
branches they are named after.  The hooks' argument checks run here too: they return before any device work."""
import numpy as np
import pytest

from oracle import refine_oracle as RO
from tests import irls_oracle as IO
from tests import laa_maps_cases as K
from tests import laa_maps_oracle as O

EPS = O.EPS


def blocks3(R):
    return np.asarray(R).reshape(-1, 3, 3).transpose(2, 1, 0)                    # (N, 9) column-major -> 3 x 3 x N


# ---------------------------------------------------------------------------------------------------------------- maps
def test_r2q_restatement_against_the_oracle_and_mpmath():
    R, labels, well = K.r2q_blocks()
    with np.errstate(all="ignore"):
        assert O.bit_equal(O.r2q_a(R), RO.R2Q(blocks3(R)))
        assert O.bit_equal(O.r2q_a(R, True), RO.R2Q(np.transpose(blocks3(R), (1, 0, 2))))
    a, b = O.r2q_a(R), O.r2q_b(R)
    ok = ~np.array([O.mp.isnan(v) for v in b[:, 0]])
    assert ok.sum() >= 140                                                      # (tr + 1) / 4 of a pi - 1e-8 rotation in double is <= 0 for some axes
    # the trace loses (tr + 1) = 4 a^2 to cancellation: |da| <= eps / a, |dx| <= eps / a^2 (+ a few eps of the divisions)
    ab = O.to_float(b[ok, 0])
    err = O.mp_abs_err(a[ok], b[ok])
    assert np.all(err <= (4 * EPS / ab ** 2 + 4 * EPS)[:, None])
    t = labels.index("half-turn diag[1, -1, -1]")                               # R2Q.m:12: 0 / 0
    assert a[t, 0] == 0.0 and np.all(np.isnan(a[t, 1:]))
    assert np.all(np.isnan(a[labels.index("-I (sqrt of a negative)")]))
    assert O.bit_equal(a[labels.index("zero")], [0.5, 0.0, 0.0, 0.0])
    t = labels.index("one NaN")
    assert np.isnan(a[t]).sum() == 1                                            # only the component that reads the NaN entry


def test_q2r_restatement_against_the_oracle_and_mpmath():
    R, _, well = K.r2q_blocks()
    Q = np.concatenate([K.q2r_quats(), O.r2q_a(R)])
    a, b = O.q2r_a(Q), O.q2r_b(Q)
    fin = np.all(np.isfinite(a), axis=1)
    with np.errstate(all="ignore"):
        ref = np.array([RO.q2R(q).reshape(9, order="F") for q in Q])
    assert np.array_equal(np.isnan(ref), np.isnan(a))
    scale = np.sum(Q ** 2, axis=1)
    scale = np.where(np.isfinite(scale), np.maximum(1.0, scale), 1.0)[:, None]          # a NaN q.a fails the `>` of q2R.m:4: identity
    assert np.all(np.abs(ref - a)[fin] <= (8 * EPS * scale * np.ones(9))[fin])  # q2R's norm() rounds differently from the explicit sum
    err = O.mp_abs_err(a[fin], b[fin])
    assert np.all(err <= (16 * EPS * scale * np.ones(9))[fin])
    ident = np.abs(np.abs(Q[:, 0]) - 1.0) <= 1e-12
    assert ident.sum() >= 5 and (~ident & (np.abs(np.abs(Q[:, 0]) - 1.0) < 3e-12)).sum() >= 2      # both sides of q2R.m:4
    assert np.all(a[ident] == np.eye(3).reshape(9))
    # the round trip of the well-conditioned rotations gives R back
    Rw = R[well]
    far = np.abs(O.r2q_a(Rw)[:, 0] - 1.0) > 1e-12                               # below ~2.8e-6 rad q2R.m:4 returns the identity: off by theta
    assert far.sum() >= 60 and (~far).sum() >= 40
    # double: the cancellation in tr + 1 = 4 a^2 leaves |da| ~ eps / a, which sin(theta) = 2 s2 a carries into R
    qa = O.r2q_a(Rw)[far, :1]
    assert np.all(np.abs(O.q2r_a(O.r2q_a(Rw)) - Rw)[far] <= 64 * EPS / qa)
    assert np.all(np.abs(O.to_float(O.q2r_b(O.r2q_b(Rw))) - Rw)[far] <= 64 * EPS / qa)       # R in double is a rotation only to rounding
    assert np.all(O.q2r_a(O.r2q_a(Rw))[~far] == np.eye(3).reshape(9))


def test_qmul_and_edge_log_restatements_against_the_oracles():
    g = np.random.default_rng(1)
    A, B = g.normal(size=(50, 4)), g.normal(size=(50, 4))
    assert O.bit_equal(O.qmul_a(A, B), RO.qmul(A, B))
    for c in K.edge_log_random() + [K.edge_log_control()]:
        I = np.stack([c["ii"] + 1, c["jj"] + 1])
        Ba = O.edge_log_a(c["ii"], c["jj"], c["Q"], c["QQ"])[0]
        assert O.bit_equal(Ba, IO.edge_log(I, c["Q"], c["QQ"]))
        A_ = RO.Build_Amatrix(I)
        assert O.bit_equal(Ba, RO.Weighted_LAA(I, c["Q"].copy(), c["QQ"], A_, np.ones(len(c["ii"])))[2])
        Bb, _ = O.edge_log_b(c["ii"], c["jj"], c["Q"], c["QQ"])
        r = O.few_ulp(Ba, Ba, Bb)
        assert r["worst_a_ulp"] < 1e9                                           # finite; the small angles are ill-conditioned by design


def test_edge_log_control_reaches_its_branches():
    c = K.edge_log_control()
    B, v, v1 = O.edge_log_a(c["ii"], c["jj"], c["Q"], c["QQ"])
    assert np.array_equal(v, c["QQ"])                                           # the alternating +-(1,0,0,0) nodes make v = QQ exactly
    lab = c["labels"]
    assert np.all(B[0] == 0) and np.all(B[1] == 0) and v1[1] == 0.0             # 2 pi wraps to 0; 0/0 -> 0
    for e, sg in enumerate(c["sign"]):
        if sg:
            assert np.sign(B[e] @ c["axis"][e]) == sg, lab[e]
    e = lab.index("angle pi+1e-09")
    assert abs(abs(v1[e]) - np.pi) < 2e-9 and v1[e] < 0 and v1[lab.index("angle pi-1e-09")] > 0
    for e in c["knife"]:                                                        # 2 * (pi / 2 rounded) == M_PI: the wrap takes it to -pi
        assert v1[e] == -np.pi, (lab[e], v1[e])
    assert v[c["knife"][1], 0] == 0 and np.signbit(v[c["knife"][1], 0])
    s2 = np.sqrt(np.sum(v[2:4, 1:] ** 2, axis=1))
    assert np.all((s2 > 0) & (s2 < 2e-160))


# ---------------------------------------------------------------------------------------------------------------- rhs, pcg
def test_rhs_restatement_against_mpmath_and_the_incidence_matrix():
    for c in K.rhs_cases():
        n, ii, jj = c["n"], c["ii"], c["jj"]
        rhs, diag = O.rhs_a(n, ii, jj, c["w"], c["B"])
        rb, db, mag, terms = O.rhs_b(n, ii, jj, c["w"], c["B"])
        assert np.all(O.mp_abs_err(rhs, rb) <= (terms[:, None] + 2) * EPS * O.to_float(mag)), c["name"]
        A = RO.Build_Amatrix(np.stack([ii + 1, jj + 1]))                        # node 1 grounded: rows 1.. of rhs
        dense = A.T @ (c["w"][:, None] ** 2 * c["B"])
        assert np.allclose(dense, rhs[1:], rtol=0, atol=1e-12 * max(1.0, np.abs(dense).max())), c["name"]
        assert np.allclose(np.diag(A.T @ (c["w"][:, None] ** 2 * A)), diag[1:], rtol=1e-13), c["name"]
        if "iso" in c:
            assert diag[c["iso"]] == 0.0
    assert max(t.max() for t in (O.rhs_b(c["n"], c["ii"], c["jj"], c["w"], c["B"])[3] for c in K.rhs_cases()[:8])) >= 33


@pytest.mark.parametrize("cases", [K.pcg_cases, K.pcg3_cases], ids=["laa", "primal-dual"])
def test_pcg_restatement_meets_the_contract(cases):
    worst_gap = worst_fe = 0.0
    for c in cases():
        n, ii, jj, w3 = c["n"], c["ii"], c["jj"], c.get("w3", False)
        ref = O.pcg_a(n, ii, jj, c["w"], c["rhs"], c["diag"], c["act"], w3=w3)
        assert ref["total"] % ref["probe"] == 0 or ref["total"] == ref["cap"]
        if c.get("zero"):
            assert np.all(ref["x"] == 0) and ref["total"] == ref["probe"] and ref["unconverged"] == 0
            continue
        if c.get("nan") is not None:
            assert ref["bad"].tolist() == [int(k == c["nan"]) for k in range(3)]
        assert ref["unconverged"] == 0, (c["name"], ref["total"])
        rt = O.true_residual_b(n, ii, jj, c["w"], c["rhs"], ref["x"], w3=w3)
        xb = None
        for k in range(3):
            if not c["act"][k] or k == c.get("nan") or k == c.get("dead"):
                continue
            bn = np.sqrt(ref["bnorm"][k])
            if bn == 0:
                continue
            gap = np.linalg.norm(rt[:, k] - ref["r"][:, k]) / bn
            worst_gap = max(worst_gap, gap)
            assert np.linalg.norm(rt[:, k]) <= (1e-13 + gap) * bn * (1 + 1e-9)
            kappa = O.jacobi_condition(n, ii, jj, c["w"][:, k] if w3 else c["w"] * c["w"])
            if kappa <= 1e6:
                xb = O.pcg_b(n, ii, jj, c["w"], c["rhs"], w3=w3) if xb is None else xb
                fe = np.linalg.norm(O.mp_abs_err(ref["x"][:, k], xb[:, k])) / np.linalg.norm(O.to_float(xb[:, k]))
                worst_fe = max(worst_fe, fe / (kappa * 1e-13))
                assert fe <= kappa * 1e-13, (c["name"], k, fe, kappa)
    print(f"[laa_maps host] restatement: worst gap / |b| = {worst_gap:.3g}, worst forward error / (kappa 1e-13) = {worst_fe:.3g}")


def test_pcg_cap_is_reachable_without_nan():
    c = K.pcg_cap_case()
    ref = O.pcg_a(c["n"], c["ii"], c["jj"], c["w"], c["rhs"], c["diag"], c["act"])
    assert ref["total"] == ref["cap"] == 240 and ref["unconverged"] == 1 and np.all(ref["x"] == 0) and np.all(np.isfinite(ref["r"]))


def test_weighted_laa_step_from_the_pieces():
    """edge_log -> rhs -> the grounded solve -> exp map -> product, assembled from this file's references, equals Weighted_LAA.m as
    oracle/refine_oracle.py restates it (lstsq in place of the sparse QR)."""
    n, ii, jj = K.complete_graph(9)
    c = K.edge_log_random()[0]
    w = 10.0 ** np.random.default_rng(2).uniform(-1, 1, size=len(ii))
    I = np.stack([ii + 1, jj + 1])
    Q1, W, B, score = RO.Weighted_LAA(I, c["Q"].copy(), c["QQ"], RO.Build_Amatrix(I), w)
    Ba = O.edge_log_a(ii, jj, c["Q"], c["QQ"])[0]
    rhs, diag = O.rhs_a(n, ii, jj, w, Ba)
    x = O.to_float(O.pcg_b(n, ii, jj, w, rhs))
    wq, th = O.qexp_a(x)
    assert np.allclose(wq, W, atol=1e-12)
    assert np.allclose(O.qmul_a(c["Q"], wq), Q1, atol=1e-12)
    assert abs(th[1:].sum() / n - score) <= 1e-12
    ref = O.pcg_a(n, ii, jj, w, rhs, diag)
    assert ref["unconverged"] == 0 and np.allclose(ref["x"], x, atol=1e-10)


# ---------------------------------------------------------------------------------------------------------------- node update, weights
def test_exp_map_restatement():
    x, Q = K.node_update_base()
    w, th = O.qexp_a(x)
    wb, thb = O.qexp_b(x)
    with np.errstate(all="ignore"):
        assert O.bit_equal(O.qmul_a(Q, w)[1:], IO.exp_update(Q, x[1:])[1:])     # exp_update grounds row 0; rows 1.. are the same text
    assert np.all(np.isfinite(w))
    under = th == 0
    assert under.sum() >= 4 and np.all(w[under] == [1.0, 0, 0, 0])              # theta = 0, also by underflow of t^2 (1e-200)
    nanrow = np.isnan(th)
    assert nanrow.sum() == 1 and np.all(w[nanrow] == 0)                         # NaN -> 0 in every component (Weighted_LAA.m:47)
    big = ~under & ~nanrow & (th > 1e-100)
    assert np.all(O.mp_abs_err(w[big], wb[big]) <= 4 * EPS)


def test_weights_restatement():
    RS = K.weights_values()
    for thresh in K.WEIGHT_THRESHOLDS:
        a, b = O.weights_a(RS, thresh), O.weights_b(RS, thresh)
        with np.errstate(all="ignore"):
            ref = 1.0 / RS ** 0.75; ref[ref > 1e4] = 1e4; ref[RS > thresh] = 1e-4          # DESC.m:298-303 as refine_oracle writes it
        assert O.bit_equal(a, ref)
        r = O.few_ulp(a, a, b)
        assert r["worst_a_ulp"] <= 2, r
    a = O.weights_a(RS, 0.5)
    assert a[RS == 0.5][0] > 1 and a[RS == np.nextafter(0.5, np.inf)][0] == 1e-4
    xc = float(O.mp.power(O.mp.mpf(10), O.mp.mpf(-16) / 3))
    near = np.abs(RS - xc) < 1e-18
    assert near.sum() == 7 and (a[near] == 1e4).any() and (a[near] < 1e4).any()          # both sides of the crossing
    assert np.isnan(a[np.isnan(RS) | ((RS < 0) & np.isfinite(RS))]).all()
    c = K.irls_weight_cases()
    for mode in (O.GM, O.L12):
        for sigma in map(np.float64, c["sigmas"]):
            a = O.irls_weights_a(c["ii"], c["jj"], c["x"], c["B"], mode, sigma)
            b = O.irls_weights_b(c["ii"], c["jj"], c["x"], c["B"], mode, sigma)
            E = np.where(c["jj"][:, None] > 0, c["x"][c["jj"]], 0) - np.where(c["ii"][:, None] > 0, c["x"][c["ii"]], 0) - c["B"]
            s = np.sum(E ** 2, axis=1)
            with np.errstate(all="ignore"):
                ref = sigma / (s + sigma ** 2) if mode == O.GM else np.minimum(1.0 / np.sqrt(s) ** 0.75, 1e4)
            fin = np.isfinite(ref) & (ref > 0) & np.isfinite(a)
            assert np.allclose(a[fin], ref[fin], rtol=1e-12)
            assert np.all(s[[10, 11, 20]] == 0)
            if 1e-100 < sigma < 1e100:
                assert O.few_ulp(a, a, b)["worst_a_ulp"] <= 8


# ---------------------------------------------------------------------------------------------------------------- quantile
def test_quantile_restatement_and_the_paths_the_cases_take():
    seen = set()
    for name, x, ps in K.quantile_data():
        for p in ps:
            a = O.quantile_a(x, p)
            ref = np.quantile(x, p, method="hazen")
            if np.isfinite(ref):
                assert abs(a - ref) <= 2 * np.spacing(abs(ref)), (name, p, a, ref)
            # (b): p m + 0.5 rounds once (relative eps / 2 of a position below m), fr (b - a) and the sum once each
            qb, lo_, hi_ = O.quantile_b(x, p)
            if np.isfinite(hi_ - lo_):
                assert abs(O.mp.mpf(float(a)) - qb) <= 2 * EPS * (abs(float(qb)) + x.size * abs(hi_ - lo_)), (name, p, a, float(qb))
            plan = O.quantile_plan(x, p)
            seen.add(plan["path"])
            if plan["path"] == "bins":
                d = plan["b1"] - plan["b0"]
                seen.add("same bin" if d == 0 else "adjacent bins" if d == 1 else "far bins" if d > 1000 else "near bins")
                if plan["last_of_bin"]: seen.add("k0 last of its bin")
                if plan["need"] > 8: seen.add("need > 8")
                if plan["need"] > 1: seen.add("need > 1")
                if "overflows" in name: seen.add("overflow" if plan["b0"] == plan["b1"] == 0 else "overflow?")
    assert {"min", "max", "const", "bins", "same bin", "adjacent bins", "far bins", "k0 last of its bin", "need > 8", "need > 1", "overflow"} <= seen, seen


# ---------------------------------------------------------------------------------------------------------------- projection
def test_projection_references():
    good = K.project_good_blocks()
    status, det, s, decided = O.project_status(good)
    assert decided.all() and set(status.tolist()) == {0, 1}
    RR = np.transpose(blocks3(good), (1, 0, 2))
    P, warned = IO.project(RR)
    assert warned == (status == 1).sum()
    b = O.to_float(O.project_b(good))
    want = np.array([P[:, :, e].reshape(9, order="F") for e in range(len(good))])
    assert np.abs(b - want).max() <= 64 * EPS * 2.4
    bad = K.project_bad_blocks()
    sb = O.project_status(bad)[0]
    assert O.project_status(bad)[3].all() and (sb == 3).sum() >= 4 and (sb == 2).sum() >= 4
    knife, exact = K.project_knife_blocks()
    st, _, sk, dec = O.project_status(knife)
    assert (~dec).sum() >= 6 and dec.sum() >= 40
    half = np.abs(sk - np.floor(sk) - 0.5).min(axis=1) <= 1e-12
    assert (half & exact).sum() >= 6
    pb = O.to_float(O.project_b(knife[half & exact]))
    for blk, pr in zip(knife[half & exact], pb):                                # half away from zero: 0.5 -> 1, 1.5 -> 2
        se = np.abs(blk[blk != 0])
        assert sorted(np.abs(pr[pr != 0]).tolist()) == sorted(np.floor(se + 0.5).tolist())


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_an_unsorted_edge_list_never_reaches_a_kernel(lib):
    """The issue's "edge list not sorted by i" for edge_log: desc_problem_upload validates the list before it looks for a device and
    refuses it, so no kernel of the core can see one."""
    for ii, jj in (([1, 0], [2, 1]), ([0, 0], [2, 1]), ([1], [0])):
        ii, jj = np.array(ii, dtype=np.int32), np.array(jj, dtype=np.int32)
        with pytest.raises(lib.DescError) as ei:
            lib.DeviceProblem(lib.ProblemArrays(3, ii, jj, K.identity_rij(len(ii))))
        assert ei.value.code == lib.ERR_INVALID


def test_hooks_refuse_bad_arguments_before_any_device_work(lib):
    L = lib.load()
    d = np.zeros(64); p = lib.ptr(d, lib.F64P)
    i32 = np.zeros(8, dtype=np.int32); pi = lib.ptr(i32, lib.I32P)
    calls = [
        L.desc_test_laa_r2q(None, 1, 0, 0, 0, p), L.desc_test_laa_r2q(p, 1, 0, 0, 0, None), L.desc_test_laa_r2q(p, -1, 0, 0, 0, p),
        L.desc_test_laa_q2r(None, 1, 0, p), L.desc_test_laa_q2r(p, -1, 0, p),
        L.desc_test_laa_edge_log(None, p, p, 3, p), L.desc_test_laa_rhs(None, p, p, 3, p, p),
        L.desc_test_laa_pcg(None, 0, p, p, p, 3, pi, p, pi, p, p, pi, pi, p),
        L.desc_test_laa_node_update(p, p, -1, 0, p, p, p), L.desc_test_laa_node_update(p, None, 1, 0, p, p, p),
        L.desc_test_irls_node_update(p, p, -1, 0, p, p), L.desc_test_irls_node_update(None, p, 1, 0, p, p),
        L.desc_test_laa_weights(p, -1, 0.5, 0, p), L.desc_test_laa_weights(None, 1, 0.5, 0, p),
        L.desc_test_irls_weights(None, p, p, 3, 0, 1.0, p),
        L.desc_test_laa_quantile(p, 4, -0.1, 8, 0, p), L.desc_test_laa_quantile(p, 4, 1.5, 8, 0, p), L.desc_test_laa_quantile(p, 4, float("nan"), 8, 0, p),
        L.desc_test_laa_quantile(p, -1, 0.5, 8, 0, p), L.desc_test_laa_quantile(p, 4, 0.5, 0, 0, p), L.desc_test_laa_quantile(None, 4, 0.5, 8, 0, p),
        L.desc_test_irls_project(None, None, 1, -1, 0, p, pi, pi, p), L.desc_test_irls_project(p, None, -1, -1, 0, p, pi, pi, p),
        L.desc_test_irls_project(p, None, 1, 1, 0, p, pi, pi, p),
        L.desc_test_irls_pd_stage(None, 0, p, p, p, pi, 1, 2, p, p, p), L.desc_test_irls_pd_solve(None, p, 1, 2, 2, p, p, pi, p, 3, pi),
    ]
    assert all(rc == lib.ERR_INVALID for rc in calls), calls
    assert L.desc_last_error()


PD_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from desc_amd import _lib as lib
from tests import laa_maps_cases as K
L = lib.load()
assert hasattr(L, "hipmock_launch_count"), "must run against the mock build"
n, ii, jj = K.path_graph(4)
dp = lib.DeviceProblem(lib.ProblemArrays(n, ii, jj, K.identity_rij(len(ii))))
m = dp.m
d = np.zeros(17 * 3 * m + 6 * 256); p = lib.ptr(d, lib.F64P)
i32 = np.zeros(8, dtype=np.int32); pi = lib.ptr(i32, lib.I32P)
h = dp.handle
stage = lambda *a: L.desc_test_irls_pd_stage(*a)
solve = lambda *a: L.desc_test_irls_pd_solve(*a)
c0 = L.hipmock_launch_count()
out = dict(
    stage_null=[stage(h, 0, *[None if k == t else (pi if k == 3 else p) for k in range(4)], m, n, p, p, p) for t in range(4)] +
               [stage(h, 0, p, p, p, pi, m, n, *[None if k == t else p for k in range(3)]) for t in range(3)],
    stage_size=[stage(h, 0, p, p, p, pi, m + 1, n, p, p, p), stage(h, 0, p, p, p, pi, m, n - 1, p, p, p), stage(h, 0, p, p, p, pi, -1, n, p, p, p)],
    stage_id=[stage(h, -1, p, p, p, pi, m, n, p, p, p), stage(h, len(lib.PD_STAGES), p, p, p, pi, m, n, p, p, p)],
    solve_null=[solve(h, None, m, n, 2, p, p, pi, p, 3, pi), solve(h, p, m, n, 2, None, p, pi, p, 3, pi), solve(h, p, m, n, 2, p, None, pi, p, 3, pi),
                solve(h, p, m, n, 2, p, p, None, p, 3, pi), solve(h, p, m, n, 2, p, p, pi, None, 3, pi), solve(h, p, m, n, 2, p, p, pi, p, 3, None)],
    solve_size=[solve(h, p, m - 1, n, 2, p, p, pi, p, 3, pi), solve(h, p, m, n + 1, 2, p, p, pi, p, 3, pi)],
    solve_iter=[solve(h, p, m, n, -1, p, p, pi, p, 3, pi)],
)
out["refused_launches"] = L.hipmock_launch_count() - c0
out["invalid"] = lib.ERR_INVALID
before = L.hipmock_launch_count()
# the wrappers end to end (no kernel runs: device blocks read back as zeros): sizes, guard words, the stage names
st = {k: np.zeros((m, 3)) for k in lib.PD_EDGE}; st.update({k: np.zeros((n, 3)) for k in lib.PD_NODE})
for s in lib.PD_STAGES:
    got, part = lib.hook_pd_stage(dp, s, st, np.zeros((lib.PD_RG, 6)))
    assert set(got) == set(lib.PD_EDGE) | set(lib.PD_NODE) and part.shape == (6 * lib.PD_RG,)
r = lib.hook_pd_solve(dp, np.zeros((m, 3)), 2)
assert r["x"].shape == (n, 3) and r["trace"].shape[1:] == (3, 8) and r["steps"] == 0
out["ok_launches"] = L.hipmock_launch_count() - before
print("RESULT " + json.dumps(out))
"""


def test_pd_hooks_refuse_bad_arguments_on_the_mock_runtime():
    """desc_test_irls_pd_stage / desc_test_irls_pd_solve on a device problem of the mock HIP runtime (tests/hipmock: no GPU): a NULL
    pointer, an m or n that is not the problem's, an unknown stage and pdmaxiter < 0 are refused with DESC_ERR_INVALID before anything
    is launched; the host build still links, and the Python wrappers run end to end."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests", "hipmock"))
    import build_host
    so = build_host.build(root, "none")
    env = dict(os.environ, DESC_AMD_LIB=so, OPENBLAS_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-c", PD_CHILD, root], env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    for key in ("stage_null", "stage_size", "stage_id", "solve_null", "solve_size", "solve_iter"):
        assert out[key] and all(rc == out["invalid"] for rc in out[key]), (key, out[key])
    assert out["refused_launches"] == 0 and out["ok_launches"] > 0

"""The Lie-algebraic averaging core (desc_amd/csrc/laa.hip, laa.h; k_irls_project / k_irls_weights / k_l1_node_update of irls.hip)
kernel by kernel, through the desc_test_laa_* / desc_test_irls_* hooks, which launch each kernel alone with the grid rule of the library.

Comparison rules
  exact    operations made of + - * / and sqrt are bit-equal to restatement (a) of tests/laa_maps_oracle.py (NaN positions and the signs
           of zeros and infinities included): both sides round correctly, any difference is a change of arithmetic.
  few-ulp  operations that call atan2 / sin / cos / pow: per component, device error against the 50-digit reference (b) <= 4 x the error
           of restatement (a) against (b) + 4 ulp of the component's magnitude (for B: of the edge's vector norm).  Where the libm result
           can be isolated the rest of the kernel is still checked exactly: edge_log must be bit-equal to (a) evaluated with atan2 moved
           by some k ulp; node_update's product must be bit-equal to qmul_a(Q, w) of the w the device returned for Q = (1,0,0,0).
  count    non-finite positions agree exactly with (a).

Case -> kernel line reached (laa.hip unless noted)
  r2q   identity / small and large angles, 23 axes         :31-33 plain path
        exact half-turns diag(1,-1,-1) and permutations    :33 x / 0 -> inf, 0 / 0 -> NaN (R2Q.m:12 divides by q(:,1) = 0: a quirk, pinned)
        half-turn about a random axis                      :32 sqrt of a value within rounding of 0 (NaN when it comes out negative)
        zero block, 2 I, -I, one NaN, one Inf, round(S)=2  :32 sqrt(0.25), sqrt(1.5), sqrt(-0.5) = NaN, NaN / Inf propagate per component
        counts 1, 255, 256, 257, 512*256+5                 :37 the grid-stride loop, partial last block, wrap of the 512-block node grid
        transpose 0 / 1, node grid / edge grid             :29 the swaps; laa_setup's ngrid and egrid
  q2r   a = +-1, +-(1-1e-13), +-(1-1e-12), +-(1-2e-12)     :45 both sides of the identity threshold (q2R.m:4)
        a = +-0 with a unit vector part; zero quaternion   :46-48 s2 = 0 -> 0/0 NaN block; unnormalised q (no renormalisation, q2R.m)
        r2q outputs of the rotations up to pi - 1e-3       :45-52 the round trip against (b) of the composition
  edge_log  v = (+-1,0,0,0)                                :65-72 s2 = 0; 2 atan2(0,-1) = 2 pi >= pi wraps to 0; 0/0 -> NaN -> 0 (:35)
        s2 = 1e-160                                        :64 s2^2 underflows to a subnormal
        angles 1e-8, pi +- 1e-9, pi +- 1e-3, v.a < 0       :66-67 the wrap: the sign of B jumps at pi (Weighted_LAA.m:27-28, pinned)
        v.a = +-0, s2 = 1                                  :65-67 2 atan2(1, +-0) against M_PI: see "knife edge" below
        complete graph on 9, path of 300                   :61 gathers by i and j; edges at node 0 and at the last node
        (an edge list not sorted by i cannot reach the kernel: desc_problem_upload refuses it -- tests/test_laa_maps_host.py pins that)
  rhs   stars of 17 / 33 spokes, hub 0 and hub last        :88 one and two / three passes of the 16-lane row loop; :94 the butterfly
        isolated node (all weights 0)                      :92 diag = 0
        weights 1e-4 next to 1e4, log-uniform              :90-91
  pcg   zero right-hand side                               :357 rnorm > 1e-300 fails at the first probe: x = 0, `probe` steps
        act masks, a zero coordinate                       :357 coordinates out of the test
        <true,true>: zero weights, NaN weight              :152 pq = 0 -> alpha = 0; :128,156 breakdown -> bad[c], alpha = 0
        single edge with diag = 0                          :341,358 the cap 20 n + 200
  node_update  theta = 0, 1e-200, 1e-160                   laa.h:74-82 t1^2 underflows: theta = 0, sin(0)/0 = NaN -> 0, w = (1,0,0,0)
        NaN row                                            laa.h:79-82 every component NaN -> 0: w = 0, Q_new = 0 (pinned as (a) gives it)
        row 0 non-zero                                     :189 moves Q[0], not in the score
        n = 1, 255, 256, 257, 64*256+3                     :186,193-197 the 64 blocks of 256 and their wrap; irls.hip:251-257 the max
  weights  RS = 0, 1e-320, crossing of 1e4, == thresh, nextafter(thresh), thresh inf / -inf / NaN, RS NaN / negative   :202-204
  irls_weights  s = 0 (both modes), sigma 1e-300 .. 1e200, node 0 grounded    irls.hip:264-268, laa.h:91
  quantile  pos <= 1, pos >= m, hi == lo                   :263-265 early returns
        k0, k0+1 in one bin / adjacent / far apart, k0 last of its bin, hi - lo overflows (scale = 0)   :273-293
        cap 8 and 1                                        :281 the exact host path (matlab_quantile)
  project  rotations; s at and around 0.5, 0.9, 0.99, 1.5; rank 1 / 2 / 0; reflections; order    irls.hip:81-103

Measured on an MI355X (gfx950; the device libm against glibc's).  Every figure is printed by the tests (run with -s).
  exact        found bit-equal to restatement (a) on every case: r2q (both orientations, both grids, up to 131 077 blocks), q2r, rhs and
               diag (the order of the 16-lane sum included), the whole Jacobi-PCG in both instances (x, |r|^2, |b|^2, steps, worst,
               bad[]), the quantile (device path and host path), node_update's product given the device's own w, Wv, the fmax score,
               weights' compare-and-clip, the GM weights, project's det / status / bad_row / warning count and the singular values of
               blocks with orthogonal columns.
  edge_log     atan2 differs from glibc's by -1, 0 or +1 ulp (69-79 % of the edges equal); with that one value moved every B is bit-equal
               to (a).  Against (b): worst device error 12.3 ulp of |B_e| where (a) itself is 14.3 ulp off (the products cancel at small
               angles); worst error / allowance 0.47.
  knife edge   v.a = +0 and -0 with s2 = 1: atan2(1, +-0) is the same double on both sides (pi / 2 rounded), twice it == M_PI, and the wrap
               `v1 >= pi` takes it: the device returns B = -pi * axis, as glibc does.  Asserted: atan2 must equal glibc's on these rows
               and B must be -pi * axis (an atan2 one ulp lower would give +pi * axis and fail).
  qexp         sin / cos: 97.5 % of the components equal to glibc's; worst error / allowance 0.25.  In ulp of the component: 0.51 on a
               generic row, and 2e16 on both sides at theta = 2 pi, where sin(theta / 2) is all cancellation.  theta = 1e-200: t^2
               underflows, w = (1, 0, 0, 0) on both sides, as the reference gives it.
  node_update  Q * w against (b): worst 0.68 ulp of 1 (the restatement: 0.68), error / allowance 0.10; the score (rows without the NaN row) is off by
               at most 1.3e-3 of (n + 2) eps sum(theta) at n = 255, 256, 257 and by 8e-5 of it at n = 16 387; n = 1 gives 0 exactly.
  weights      pow: worst 1.25 ulp (glibc: 1.24), error / allowance 0.25; 83-87 % of the values equal to glibc's.
  irls_weights L12 (sqrt, pow): worst 2.25 ulp (restatement: 1.25), error / allowance 0.45.
  round trip   q2r(r2q(R)), theta <= pi - 1e-3: bit-equal to (a); 1.6 ulp of 1 from (b) of the composition, error / allowance 0.15.
               |q2r(r2q(R)) - R| reaches theta itself (1e-8) below 2.8e-6 rad, where q2R.m:4 returns the identity: pinned.
  rhs          worst error / ((terms + 2) eps sum |w^2 B|) = 0.26.
  pcg          |r_true - r_recurrence| / |b|, the gap the contract |r| <= 1e-13 |b| is read up to: at most 1.3e-11 in the primal-dual
               instance (weights over 4 decades), but 5.77 in Weighted_LAA's instance on the path of 40 with weights log-uniform in
               [1e-4, 1e4] (operator weights w^2 over 16 decades): the solve reports convergence while b - A'W^2 A x is 5.8 |b|.  That
               is the floor eps |A| |x| of the normal equations in double, not an error of the kernels -- the restatement has the same
               bits -- but a converged count says little about such a system.  Forward error where kappa <= 1e6: at most 1.8e-15 |x|
               (kappa up to 2578) and 8.0e-15 |x| (primal-dual, kappa up to 5.2e5).  The cap min(20000, 20 n + 200) = 240 is reached
               on the single-edge graph with a zero Jacobi diagonal (alpha stays 0: no NaN, no progress).
  project      P against mpmath's U round(S) V': worst 0.56 of 16 eps max(s), and 0.54 of it over the 27 blocks whose
               max(s) < 1 (0.4999 R .. 0.991 R, where the bound is smallest).  18 of the 82 threshold blocks have a singular value
               within 1e-12 of a status threshold (status not asserted), 6 rotated ones within 1e-12 of a half-integer (P not
               compared); with orthogonal columns round(0.5) = 1 and round(1.5) = 2 (half away from zero) are asserted.
  quantile     cap 8 sends 49 of the cases to the exact host path, cap 1 sends 101, cap 2^20 none.
  not reached  an edge list not sorted by i (desc_problem_upload refuses it before any kernel runs).
"""
import numpy as np
import pytest

from tests import laa_maps_cases as K
from tests import laa_maps_oracle as O

pytestmark = pytest.mark.gpu

EPS = O.EPS


def report(name, **kv):
    print(f"[laa_maps] {name}: " + ", ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def upload(lib, n, ii, jj):
    return lib.DeviceProblem(lib.ProblemArrays(n, ii, jj, K.identity_rij(len(ii))))


def assert_few_ulp(name, dev, a, b, mag=None):
    r = O.few_ulp(dev, a, b, mag)
    report(name, worst_ratio=r["worst_ratio"], worst_ulp=r["worst_ulp"], restatement_ulp=r["worst_a_ulp"],
           bit_equal_to_glibc=float(np.mean(np.asarray(dev).view(np.uint64) == np.asarray(a, dtype=np.float64).view(np.uint64))))
    assert r["nonfinite_same"], f"{name}: non-finite positions differ from restatement (a)"
    assert r["ok"], f"{name}: worst error / allowance {r['worst_ratio']:.3g} at {r['where'][:5].tolist()}"
    return r


# ================================================================================================================ r2q / q2r
@pytest.fixture(scope="module")
def blocks():
    R, labels, well = K.r2q_blocks()
    return R, labels, well


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("count", K.R2Q_COUNTS)
def test_r2q_is_bit_equal_to_the_restatement(lib, blocks, count, transpose):
    R = K.tiled(blocks[0], count)
    for edge_grid in (False, True):
        got = lib.hook_r2q(R, transpose=transpose, edge_grid=edge_grid)
        want = O.r2q_a(R, transpose)
        if not O.bit_equal(got, want):
            bad = [blocks[1][t % len(blocks[1])] for t in range(count) if not O.bit_equal(got[t], want[t])][:5]
            raise AssertionError(f"count {count}, transpose {transpose}, edge grid {edge_grid}: differs at {bad}")


def test_r2q_half_turn_quirk_is_carried_over(lib, blocks):
    """R2Q.m:12 divides the vector part by q(:,1) = 0 at an exact half-turn: 0/0 = NaN, x/0 = inf.  Pinned, not fixed."""
    R, labels, _ = blocks
    t = labels.index("half-turn diag[1, -1, -1]")
    q = lib.hook_r2q(R[t:t + 1])[0]
    assert q[0] == 0.0 and np.all(np.isnan(q[1:]))
    t = labels.index("-I (sqrt of a negative)")
    assert np.all(np.isnan(lib.hook_r2q(R[t:t + 1])[0]))


@pytest.mark.parametrize("count", [1, 255, 256, 257, "every case"])
def test_q2r_is_bit_equal_to_the_restatement(lib, blocks, count):
    """The counts take the head of the case list (the threshold quaternions first); "every case" runs the whole list once."""
    Q = np.concatenate([K.q2r_quats(), O.r2q_a(blocks[0]), O.r2q_a(blocks[0], True)])
    assert len(Q) > 257
    Q = Q if count == "every case" else Q[:count]
    got, want = lib.hook_q2r(Q), O.q2r_a(Q)
    if not O.bit_equal(got, want):
        bad = [t for t in range(len(Q)) if not O.bit_equal(got[t], want[t])][:5]
        raise AssertionError(f"differs at rows {bad}: {Q[bad[0]]}")
    ident = np.abs(np.abs(Q[:, 0]) - 1.0) <= 1e-12
    assert np.all(got[ident] == np.eye(3).reshape(9))


def test_round_trip_against_the_composition(lib, blocks):
    """q2r(r2q(R)) of the rotations up to pi - 1e-3 against (b) of the composition (no rounding between the two maps)."""
    R = blocks[0][blocks[2]]
    got = lib.hook_q2r(lib.hook_r2q(R))
    a = O.q2r_a(O.r2q_a(R))
    b = O.q2r_b(O.r2q_b(R))
    assert O.bit_equal(got, a)
    r = assert_few_ulp("round trip q2r(r2q(R))", got, a, b, mag=1.0)
    err_R = np.abs(got - R).max()
    report("round trip |q2r(r2q(R)) - R|", max_abs=float(err_R))


# ================================================================================================================ edge_log
def _edge_log_exact_given_atan2(got, c):
    """Every row must be bit-equal to (a) with atan2 moved by some k ulp, |k| <= 8: everything but the libm call is exact.  -> the k's."""
    ks = np.full(len(c["ii"]), 99)
    for k in sorted(range(-8, 9), key=abs):
        Bk = O.edge_log_a(c["ii"], c["jj"], c["Q"], c["QQ"], atan_shift=k)[0]
        hit = np.array([O.bit_equal(got[e], Bk[e]) for e in range(len(ks))])
        ks = np.where((ks == 99) & hit, k, ks)
    return ks


def test_edge_log_branches(lib):
    c = K.edge_log_control()
    dp = upload(lib, c["n"], c["ii"], c["jj"])
    got = lib.hook_edge_log(dp, c["Q"], c["QQ"])
    dp.free()
    a, v, v1 = O.edge_log_a(c["ii"], c["jj"], c["Q"], c["QQ"])
    b, _ = O.edge_log_b(c["ii"], c["jj"], c["Q"], c["QQ"])
    assert np.array_equal(v, c["QQ"])                                         # the construction: v is the wanted quaternion
    knife = np.zeros(len(a), dtype=bool); knife[c["knife"]] = True
    # the knife edge: v.a = +-0, s2 = 1 -> 2 atan2(1, +-0) compared with M_PI decides between +pi and -pi on the last bit of atan2
    for e in c["knife"]:
        report(f"knife edge {c['labels'][e]}", device_B=got[e].tolist(), glibc_B=a[e].tolist(), same=O.bit_equal(got[e], a[e]))
    ks = _edge_log_exact_given_atan2(got, c)
    report("edge_log control: atan2 shift against glibc", shifts=sorted(set(ks.tolist())))
    assert np.all(ks != 99), f"not explained by an atan2 difference: {[c['labels'][e] for e in np.flatnonzero(ks == 99)]}"
    # atan2(1, +-0) was measured to be pi / 2 rounded on the card, as in glibc: twice it == M_PI, `v1 >= M_PI` wraps it, and B is -pi
    # times the axis (+pi would mean an atan2 one ulp lower: k = -1).  Weighted_LAA.m:27-28 jumps here; the value is pinned.
    assert np.all(ks[c["knife"]] == 0), ks[c["knife"]]
    for e in c["knife"]:
        assert np.array_equal(got[e], -np.pi * c["QQ"][e, 1:]), (c["labels"][e], got[e])      # zeros of either sign
    assert_few_ulp("edge_log control", got[~knife], a[~knife], b[~knife], mag=np.linalg.norm(O.to_float(b[~knife]), axis=1, keepdims=True))
    for e, sg in enumerate(c["sign"]):
        if sg is None:
            continue
        d = float(got[e] @ c["axis"][e])
        assert (d == 0.0 and np.all(got[e] == 0.0)) if sg == 0 else np.sign(d) == sg, (c["labels"][e], got[e])
    assert np.all(np.isfinite(got))


@pytest.mark.parametrize("which", [0, 1], ids=["K9", "path300"])
def test_edge_log_random_graphs(lib, which):
    c = K.edge_log_random()[which]
    dp = upload(lib, c["n"], c["ii"], c["jj"])
    got = lib.hook_edge_log(dp, c["Q"], c["QQ"])
    dp.free()
    a = O.edge_log_a(c["ii"], c["jj"], c["Q"], c["QQ"])[0]
    b, _ = O.edge_log_b(c["ii"], c["jj"], c["Q"], c["QQ"])
    ks = _edge_log_exact_given_atan2(got, c)
    report("edge_log random: atan2 shift against glibc", shifts=sorted(set(ks.tolist())), share_equal=float(np.mean(ks == 0)))
    assert np.all(ks != 99)
    assert_few_ulp("edge_log random", got, a, b, mag=np.linalg.norm(O.to_float(b), axis=1, keepdims=True))


# ================================================================================================================ rhs
@pytest.fixture(scope="module")
def rhs_refs():
    out = []
    for c in K.rhs_cases():
        out.append((c, O.rhs_a(c["n"], c["ii"], c["jj"], c["w"], c["B"]), O.rhs_b(c["n"], c["ii"], c["jj"], c["w"], c["B"])))
    return out


def test_rhs_and_diagonal(lib, rhs_refs):
    worst = 0.0
    for c, (rhs_a, diag_a), (rhs_b, diag_b, mag, terms) in rhs_refs:
        dp = upload(lib, c["n"], c["ii"], c["jj"])
        rhs, diag = lib.hook_rhs(dp, c["w"], c["B"])
        dp.free()
        # exact: the products and the kernel's own order of the 16-lane sum
        assert O.bit_equal(rhs, rhs_a) and O.bit_equal(diag, diag_a), c["name"]
        # the standard summation bound against (b)
        bound = (terms[:, None] + 2) * EPS * O.to_float(mag)
        err = O.mp_abs_err(rhs, rhs_b)
        assert np.all(err <= bound), c["name"]
        worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1.0))))
        assert np.all(O.mp_abs_err(diag, diag_b) <= (terms + 2) * EPS * O.to_float(diag_b)), c["name"]
        if "iso" in c:
            assert diag[c["iso"]] == 0.0 and np.all(rhs[c["iso"]] == 0.0)
    report("rhs", worst_error_over_bound=worst)


# ================================================================================================================ pcg
def _check_pcg(lib, c, gaps):
    n, ii, jj, w3 = c["n"], c["ii"], c["jj"], c.get("w3", False)
    dp = upload(lib, n, ii, jj)
    got = lib.hook_pcg(dp, c["w"], c["rhs"], c["diag"], c["act"], w3=w3)
    dp.free()
    ref = O.pcg_a(n, ii, jj, c["w"], c["rhs"], c["diag"], c["act"], w3=w3)
    name = c["name"]
    probe, cap = ref["probe"], ref["cap"]
    assert got["total"] % probe == 0 or got["total"] == cap, (name, got["total"])
    live = [k for k in range(3) if c["act"][k] and k != c.get("nan")]
    dead = c.get("dead")
    for k in range(3):                                                         # the broken coordinate's x is not read by the caller (irls.hip: act = 0)
        if k != c.get("nan"):
            assert np.all(np.isfinite(got["x"][:, k])) and got["x"][0, k] == 0.0, name
    if c.get("zero"):
        assert np.all(got["x"] == 0.0) and got["unconverged"] == 0 and got["total"] == probe and not got["bad"].any(), (name, got)
        return
    if dead is not None:
        assert np.all(got["x"][:, dead] == 0.0), name
    if c.get("nan") is not None:
        assert got["bad"].tolist() == [int(k == c["nan"]) for k in range(3)], (name, got["bad"])
    else:
        assert not got["bad"].any(), (name, got["bad"])
    # exact: the whole solve is + - * /, and restatement (a) follows the kernels' order of summation (16 lanes and butterfly, the dots' tree)
    assert np.array_equal(got["bad"], ref["bad"]) and (got["total"], got["unconverged"]) == (ref["total"], ref["unconverged"]), (name, got, ref["total"])
    keep = [k for k in range(3) if k != c.get("nan")]
    assert O.bit_equal(got["x"][:, keep], ref["x"][:, keep]), name
    assert O.bit_equal(got["rnorm"][keep], ref["rnorm"][keep]) and O.bit_equal(got["bnorm"], ref["bnorm"]) and got["worst"] == ref["worst"], name
    if got["unconverged"]:
        report(f"pcg {name}: stopped at the cap", total=got["total"], worst=got["worst"], restatement_total=ref["total"])
        return
    # the header's contract |r| <= 1e-13 |b| on the true residual, up to the gap between the recurrence and the true residual as the
    # float64 restatement of the same recurrence shows it (x 4)
    wc = lambda k: (c["w"][:, k] if w3 else c["w"] * c["w"])      # noqa: E731
    r_dev = O.true_residual_b(n, ii, jj, c["w"], c["rhs"], got["x"], w3=w3)
    r_ref = O.true_residual_b(n, ii, jj, c["w"], c["rhs"], ref["x"], w3=w3)
    bnorm = np.sqrt(got["bnorm"])
    xb = None
    for k in live:
        if k == dead:
            continue
        gap = float(np.linalg.norm(r_ref[:, k] - ref["r"][:, k]))
        true = float(np.linalg.norm(r_dev[:, k]))
        gaps.append((name, k, gap / bnorm[k] if bnorm[k] > 0 else 0.0, true / bnorm[k] if bnorm[k] > 0 else 0.0))
        assert got["bnorm"][k] == pytest.approx(float(np.sum(c["rhs"][1:, k] ** 2)), rel=1e-14), name
        assert got["rnorm"][k] <= 1e-26 * got["bnorm"][k] or got["rnorm"][k] <= 1e-300, name
        assert true <= 1e-13 * bnorm[k] + 4 * gap, (name, k, true / bnorm[k], gap / bnorm[k])
        kappa = O.jacobi_condition(n, ii, jj, wc(k))
        if kappa <= 1e6:
            if xb is None:
                xb = O.pcg_b(n, ii, jj, c["w"], c["rhs"], w3=w3)
            xf = O.to_float(xb[:, k])
            fe = float(np.linalg.norm(O.mp_abs_err(got["x"][:, k], xb[:, k])))
            assert fe <= 4 * kappa * 1e-13 * np.linalg.norm(xf), (name, k, fe, kappa)
            gaps.append((name + " forward", k, kappa, fe / max(np.linalg.norm(xf), 1e-300)))


def test_pcg_weighted_laa_instance(lib):
    gaps = []
    for c in K.pcg_cases():
        _check_pcg(lib, c, gaps)
    res = [g for g in gaps if not g[0].endswith("forward")]
    fwd = [g for g in gaps if g[0].endswith("forward")]
    report("pcg <false,false>", worst_gap_over_b=max(g[2] for g in res), worst_true_residual_over_b=max(g[3] for g in res),
           worst_forward_error=max(g[3] for g in fwd), largest_kappa_checked=max(g[2] for g in fwd))


def test_pcg_primal_dual_instance(lib):
    gaps = []
    for c in K.pcg3_cases():
        _check_pcg(lib, c, gaps)
    res = [g for g in gaps if not g[0].endswith("forward")]
    fwd = [g for g in gaps if g[0].endswith("forward")]
    report("pcg <true,true>", worst_gap_over_b=max(g[2] for g in res), worst_true_residual_over_b=max(g[3] for g in res),
           worst_forward_error=max(g[3] for g in fwd) if fwd else 0.0, largest_kappa_checked=max(g[2] for g in fwd) if fwd else 0.0)


def test_pcg_iteration_cap(lib):
    """min(20000, 20 n + 200) = 240 steps on the single-edge graph: a zero Jacobi diagonal keeps alpha = 0 (no NaN, no progress)."""
    c = K.pcg_cap_case()
    ref = O.pcg_a(c["n"], c["ii"], c["jj"], c["w"], c["rhs"], c["diag"], c["act"])
    assert ref["total"] == 240 and ref["unconverged"] == 1
    dp = upload(lib, c["n"], c["ii"], c["jj"])
    got = lib.hook_pcg(dp, c["w"], c["rhs"], c["diag"], c["act"])
    dp.free()
    assert got["total"] == 240 and got["unconverged"] == 1 and got["worst"] == 1.0 and not got["bad"].any()
    assert np.all(got["x"] == 0.0) and np.array_equal(got["rnorm"], got["bnorm"])


# ================================================================================================================ node update
@pytest.fixture(scope="module")
def node_refs():
    x, Q = K.node_update_base()
    w_a, th_a = O.qexp_a(x)
    w_b, th_b = O.qexp_b(x)
    return dict(x=x, Q=Q, w_a=w_a, th_a=th_a, w_b=w_b, th_b=th_b, Qn_b=O.qmul_rows_b(Q, w_b))


@pytest.mark.parametrize("l1", [False, True], ids=["laa", "irls"])
@pytest.mark.parametrize("n", K.NODE_COUNTS)
def test_node_update(lib, node_refs, n, l1):
    r = node_refs
    x, Q = K.tiled(r["x"], n), K.tiled(r["Q"], n)
    rows = np.arange(n) % len(r["x"])
    ident = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    w_dev, Wv0, sc0 = lib.hook_node_update(x, ident, l1=l1)               # Q = (1,0,0,0): the product returns w itself
    Qn, Wv, score = lib.hook_node_update(x, Q, l1=l1)
    # exact: the quaternion product, on the w the device computed; Wv is w's vector part; NaN -> 0 leaves nothing non-finite
    assert O.bit_equal(Qn, O.qmul_a(Q, w_dev))
    if not l1:
        assert O.bit_equal(Wv, w_dev[:, 1:]) and O.bit_equal(Wv0, Wv)
    assert np.all(np.isfinite(Qn)) and O.bit_equal(score, sc0)
    # count / pinned rows: theta = 0 (also by underflow) gives w = (1,0,0,0); a NaN row gives w = 0
    w_a = r["w_a"][rows]
    assert np.array_equal(w_dev == 0.0, w_a == 0.0)
    under = r["th_a"][rows] == 0.0
    assert np.all(w_dev[under] == [1.0, 0.0, 0.0, 0.0])
    # few-ulp: sin / cos
    keep = np.unique(rows, return_index=True)[1]
    assert_few_ulp(f"qexp n={n}", w_dev[keep], w_a[keep], r["w_b"][rows[keep]])
    big = keep[r["th_a"][rows[keep]] > 1e-100]                                  # without the rows whose t^2 underflows (both sides lose them alike)
    assert_few_ulp(f"qexp n={n}, theta > 1e-100", w_dev[big], w_a[big], r["w_b"][rows[big]])
    assert_few_ulp(f"node_update Q n={n}", Qn[keep], O.qmul_a(Q, w_a)[keep], r["Qn_b"][rows[keep]], mag=1.0)
    # the score: theta is + * sqrt only, so each term is (a)'s; sum over v >= 1 (NaN rows excluded by neither side: the NaN row's theta is NaN)
    th = r["th_a"][rows].copy(); th[0] = 0.0
    if l1:
        assert score == float(np.fmax.reduce(th, initial=0.0))              # fmax skips NaN: exact
    else:
        fin = np.isfinite(th)
        if not fin.all():
            assert np.isnan(score)                                          # the NaN row's theta is summed as the reference sums it
        else:
            total = float(sum(r["th_b"][k] for k in rows[1:]))
            assert abs(score - total) <= (n + 2) * EPS * total


@pytest.mark.parametrize("n", K.NODE_COUNTS)
def test_node_update_score_without_nan_rows(lib, node_refs, n):
    """The fixed-order sum of the score (64 blocks of 256, four waves each) against (b) at (n + 2) eps sum(theta), on the rows without
    the NaN row (with it the score is NaN at every n >= 13: test_node_update)."""
    r = node_refs
    good = np.all(np.isfinite(r["x"]), axis=1)
    x, Q = K.tiled(r["x"][good], n), K.tiled(r["Q"][good], n)
    rows = np.arange(n) % int(good.sum())
    _, _, score = lib.hook_node_update(x, Q)
    th_b = r["th_b"][good]
    cnt = np.bincount(rows[1:], minlength=len(th_b))
    total = sum(int(cnt[k]) * th_b[k] for k in range(len(th_b)))
    err = abs(O.mp.mpf(score) - total)
    report(f"node_update score n={n}", error_over_bound=float(err / ((n + 2) * EPS * total)) if total else float(err))
    assert err <= (n + 2) * EPS * total
    assert (score > 0) == (n > 1)
    _, _, smax = lib.hook_node_update(x, Q, l1=True)
    assert smax == float(np.max(O.qexp_a(x)[1][1:], initial=0.0))


# ================================================================================================================ weights
@pytest.mark.parametrize("thresh", K.WEIGHT_THRESHOLDS, ids=lambda t: f"thresh={t}")
def test_weights(lib, thresh):
    RS = K.weights_values()
    got = lib.hook_weights(RS, thresh)
    a, b = O.weights_a(RS, thresh), O.weights_b(RS, thresh)
    # exact: the compare-and-clip logic
    cut = RS > thresh
    assert np.all(got[cut] == 1e-4)
    assert np.array_equal(np.isnan(got), np.isnan(a))                        # pow of a NaN / negative RS: NaN, never clipped
    assert np.all(got[~cut & ~np.isnan(got)] <= 1e4)
    assert np.all(got[~cut & (RS == 0)] == 1e4) and np.all(got[~cut & (RS > 0) & (RS < 1e-300)] == 1e4)
    if thresh == 0.5:
        assert got[RS == 0.5][0] > 1.0                                        # `>` is strict: RS == thresh keeps its weight (1.68)
        assert got[RS == np.nextafter(0.5, np.inf)] == 1e-4
    assert_few_ulp(f"weights thresh={thresh}", got, a, b)


@pytest.mark.parametrize("mode", [O.GM, O.L12], ids=["GM", "L12"])
def test_irls_weights(lib, mode):
    c = K.irls_weight_cases()
    dp = upload(lib, c["n"], c["ii"], c["jj"])
    for sigma in c["sigmas"]:
        got = lib.hook_irls_weights(dp, c["x"], c["B"], mode, sigma)
        a = O.irls_weights_a(c["ii"], c["jj"], c["x"], c["B"], mode, sigma)
        if mode == O.GM:
            assert O.bit_equal(got, a), sigma                                  # + * / only
        else:
            assert np.all(got[[10, 11, 20]] == 1e4)                            # s = 0: 1 / 0 = inf -> 1e4
            assert_few_ulp(f"irls_weights L12 sigma={sigma}", got, a, O.irls_weights_b(c["ii"], c["jj"], c["x"], c["B"], mode, sigma))
    dp.free()


# ================================================================================================================ quantile
@pytest.mark.parametrize("cap", K.QUANTILE_CAPS, ids=lambda c: f"cap={c}")
def test_quantile(lib, cap):
    fallback = 0
    for name, x, ps in K.quantile_data():
        if cap != K.QUANTILE_CAPS[0] and x.size > 5000:
            continue
        for p in ps:
            got = lib.hook_quantile(x, p, cap=cap)
            want = O.quantile_a(x, p)
            assert O.bit_equal(got, want), (name, p, got, want)
            ref = np.quantile(x, p, method="hazen")
            if np.isfinite(ref):
                assert abs(got - ref) <= 2 * np.spacing(abs(ref)), (name, p, got, ref)
            plan = O.quantile_plan(x, p)
            fallback += plan["path"] == "bins" and plan["need"] > cap
    report(f"quantile cap={cap}", host_path_cases=int(fallback))
    assert (fallback > 0) == (cap != K.QUANTILE_CAPS[0])


# ================================================================================================================ projection
def _check_P(name, rij, P, skip=None):
    status, det, s, decided = O.project_status(rij)
    b = O.project_b(rij)
    half = np.abs(s - np.floor(s) - 0.5).min(axis=1) <= 1e-12                 # a singular value on a rounding boundary: round() is undecided
    keep = ~half if skip is None else ~half | skip
    err = O.mp_abs_err(P, b)
    bound = 16 * EPS * s.max(axis=1)[:, None]                                  # the zero block: P must be exactly 0
    with np.errstate(all="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)[keep]
    small = (s.max(axis=1) < 1.0)[keep]
    report(f"project P {name}", worst_error_over_bound=float(ratio.max(initial=0.0)), compared=int(keep.sum()), of=len(keep),
           worst_where_max_s_below_1=float(ratio[small].max(initial=0.0)), blocks_with_max_s_below_1=int(small.sum()))
    assert np.all(err[keep] <= bound[keep]), (name, np.argwhere(~(err <= bound) & keep[:, None])[:5].tolist())


def test_project_good_blocks(lib):
    rij = K.project_good_blocks()
    status, det, s, decided = O.project_status(rij)
    assert decided.all() and status.max() <= 1
    out = lib.hook_project(rij)
    assert out["bad_row"] == -1 and out["warn"] == int((status == 1).sum())
    _check_P("good", rij, out["P"])
    order = np.random.default_rng(3).permutation(len(rij)).astype(np.int32)
    again = lib.hook_project(rij, order=order)
    assert again["bad_row"] == -1 and again["warn"] == out["warn"] and O.bit_equal(again["P"], out["P"])
    for e in (0, len(rij) - 1, int(np.flatnonzero(status == 1)[0])):
        info = lib.hook_project(rij, only=e)["info"]
        assert info[0] == status[e] and O.bit_equal(info[1], det[e])
        assert np.all(np.abs(info[2:] - s[e]) <= 16 * EPS * s[e].max())


def test_project_failures_and_the_smallest_row(lib):
    good, bad = K.project_good_blocks()[:20], K.project_bad_blocks()
    sb, detb, s_b, decided = O.project_status(bad)
    assert decided.all() and (sb >= 2).sum() >= 10 and (sb == 3).sum() >= 4 and (sb == 2).sum() >= 4
    for e in range(len(bad)):                                                  # each block alone among good ones: its status, det and s
        rij = np.concatenate([good[:7], bad[e:e + 1], good[7:]])
        out = lib.hook_project(rij, only=7)
        assert out["bad_row"] == (7 if sb[e] >= 2 else -1) and out["info"][0] == sb[e] and O.bit_equal(out["info"][1], detb[e]), (e, out["info"], sb[e])
        assert np.all(np.abs(out["info"][2:] - s_b[e]) <= 16 * EPS * max(s_b[e].max(), 1.0))
    rij = np.concatenate([good[:5], bad[:3], good[5:], bad[3:]])
    fails = np.flatnonzero(O.project_status(rij)[0] >= 2)
    out = lib.hook_project(rij)
    assert out["bad_row"] == fails.min() == 5
    order = np.random.default_rng(4).permutation(len(rij)).astype(np.int32)
    out = lib.hook_project(rij, order=order)
    assert out["bad_row"] == int(order[fails].min())                           # the smallest CALLER row
    _check_P("bad", rij, out["P"])


def test_project_on_the_thresholds(lib):
    rij, exact = K.project_knife_blocks()
    status, det, s, decided = O.project_status(rij)
    out = lib.hook_project(rij)
    # exact blocks (orthogonal columns: no Jacobi rotation, s = the column norms exactly): round() half away from zero is pinned
    _check_P("thresholds", rij, out["P"], skip=exact)
    undecided = 0
    for e in range(len(rij)):
        info = lib.hook_project(rij, only=e)["info"]
        if decided[e]:
            assert info[0] == status[e], (e, info, s[e])
        else:
            undecided += 1
        if exact[e]:                                                           # s = the column norms, exactly; the status as the kernel's compares give it
            se = np.sort(np.abs(rij[e][rij[e] != 0]))
            assert O.bit_equal(np.sort(info[2:]), se), (e, info, se)
            d = np.abs(se - 1.0)
            assert info[0] == (2 if np.all(d >= 0.1) else 1 if np.all(d >= 0.01) else 0), (e, info)
    report("project thresholds", undecided=undecided, of=len(rij))


# ================================================================================================================ arguments
def test_bad_arguments_are_refused_before_any_device_work(lib):
    L = lib.load()
    d = np.zeros(64)
    p = lib.ptr(d, lib.F64P)
    i32 = np.zeros(8, dtype=np.int32)
    pi = lib.ptr(i32, lib.I32P)
    n, ii, jj = K.path_graph(3)
    dp = upload(lib, n, ii, jj)
    h = dp.handle
    calls = [
        L.desc_test_laa_r2q(None, 1, 0, 0, 0, p), L.desc_test_laa_r2q(p, 1, 0, 0, 0, None), L.desc_test_laa_r2q(p, -1, 0, 0, 0, p),
        L.desc_test_laa_q2r(None, 1, 0, p), L.desc_test_laa_q2r(p, -1, 0, p),
        L.desc_test_laa_edge_log(None, p, p, 3, p), L.desc_test_laa_edge_log(h, p, p, 2, p), L.desc_test_laa_edge_log(h, None, p, 3, p),
        L.desc_test_laa_rhs(h, p, p, 4, p, p), L.desc_test_laa_rhs(h, p, None, 3, p, p),
        L.desc_test_laa_pcg(h, 0, p, p, p, 2, pi, p, pi, p, p, pi, pi, p), L.desc_test_laa_pcg(h, 0, p, p, p, 3, None, p, pi, p, p, pi, pi, p),
        L.desc_test_laa_node_update(p, p, -1, 0, p, p, p), L.desc_test_laa_node_update(p, None, 1, 0, p, p, p),
        L.desc_test_irls_node_update(p, p, -1, 0, p, p), L.desc_test_irls_node_update(None, p, 1, 0, p, p),
        L.desc_test_laa_weights(p, -1, 0.5, 0, p), L.desc_test_laa_weights(None, 1, 0.5, 0, p),
        L.desc_test_irls_weights(h, p, p, 2, 0, 1.0, p), L.desc_test_irls_weights(h, p, p, 3, 7, 1.0, p), L.desc_test_irls_weights(None, p, p, 3, 0, 1.0, p),
        L.desc_test_laa_quantile(p, 4, -0.1, 8, 0, p), L.desc_test_laa_quantile(p, 4, 1.5, 8, 0, p), L.desc_test_laa_quantile(p, 4, float("nan"), 8, 0, p),
        L.desc_test_laa_quantile(p, -1, 0.5, 8, 0, p), L.desc_test_laa_quantile(p, 4, 0.5, 0, 0, p), L.desc_test_laa_quantile(None, 4, 0.5, 8, 0, p),
        L.desc_test_irls_project(None, None, 1, -1, 0, p, pi, pi, p), L.desc_test_irls_project(p, None, -1, -1, 0, p, pi, pi, p),
        L.desc_test_irls_project(p, None, 1, 1, 0, p, pi, pi, p),
    ]
    dp.free()
    assert all(rc == lib.ERR_INVALID for rc in calls), calls
    assert L.desc_last_error()

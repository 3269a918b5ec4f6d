"""Restatement (a) of the primal-dual L1 solver (tests/pd_oracle.py) qualified without a GPU, on the cases of tests/pd_cases.py that
tests/test_gpu_pd_kernels.py and tests/test_gpu_pd_solver.py then hold the device to, bit for bit.

Against the reference text.  tests/irls_oracle.py's l1decode_pd (dense LU with rcond) on B = the edge log map at the spanning-tree start of
Uniform_Topology graphs with 8 / 12 / 16 / 30 nodes (seed 1), coordinate by coordinate, pdmaxiter 1, 2 and 8: the step counts are equal
(3, 6 and 24 over the three coordinates) and x agrees to 4e-18 .. 3.2e-15 at one and two steps and to 1.6e-12 at eight (12 nodes;
1.1e-16 .. 8.9e-16 on the other three graphs), under the 1e-9 tests/test_gpu_irls.py uses for this pair of solvers.
At pdmaxiter = 64 the two sides leave through different doors, as expected of a CG against an LU, and nothing is asserted:
    graph   (a): each coordinate's end, at step      LU restatement: each coordinate's end, after steps
    u8      ill 18, ill 14, ill 15                   ill after 15, 12, 13
    u12     ill 13, ill 13, ill 12                   ill after 13, 10, 15
    u16     ill 23, ill 17, ill 16                   ill after 21, 14, 18
    u30     ill 20, ill 20, ill 20                   ill after 18, 18, 17
((a)'s "ill" is the CG's breakdown, the LU's is rcond < 1e-14; the step given for (a) is the one whose solve broke down.)

Against (b).  The formulas of k_pd_pre, k_pd_dir and both k_pd_resid variants at the states (a) reaches in steps 1, 2 and 5 of the 12-node
case against the same formulas in mpmath at 50 digits, by the allowance rule of laa_maps_oracle.few_ulp with (a) in the device's place:
the error of (a) in ulp of the magnitude the formula's roundings scale with (the sum of the absolute values of its terms).  A rounding
is at most one ulp of that magnitude, and at most 16 roundings reach an output of pre, 32 one of dir (counting those inherited from
du, which dir forms first): these are the bounds asserted.  Measured: pre 1.17 ulp, dir 1.83 ulp.  The residual sums are held to
(terms + 8) eps of the sum of the terms' magnitudes (measured: 0.0068 of it).

The exit search.  Restatement (a) over SEARCH_SPACE of tests/pd_cases.py: the graphs u8, u12, u16, u30 and the complete graph on 6, seeds
0-9, B scaled by 1, 1e-3 and 1e3, pdmaxiter = 64 (150 solves, two and a half minutes).  With B or 1e3 B (100 solves, 300 coordinates)
287 coordinates end by a CG breakdown and 13 "stuck", between steps 11 and 45, and 80 of the solves have a Newton solve stopped at the
CG cap on the way; with 1e-3 B (150 coordinates) 114 end "stuck", 30 by a CG breakdown and 6 run to step 64.  In 145 of the 150 solves
the three coordinates end at different steps.  First cases, recorded in FOUND:
    a coordinate stuck while another goes on      u8 seed 1, 1e-3 B: coordinate 0 stuck in step 19, the other two take part in step 20
    a CG breakdown on finite data                 u8 seed 0, B: coordinate 0 in step 11, coordinate 2 goes on to step 13
    three different numbers of trials in a step   u8 seed 0, 1e-3 B: step 13 takes 28, 1 and 4 trials
    a step at the CG cap                          u8 seed 0, B: step 12 stops at 20 n + 200 = 360 CG steps, unconverged
    sdg < tol                                     by NO case of the space: the complementarity gap never falls under eps before a
                                                  breakdown or the 32-trial limit ends the coordinate.  That arm of pd_goes_on is
                                                  covered by the rule alone, restated against a hand-worked table below."""
import math

import numpy as np
import pytest

from tests import irls_oracle as IO
from tests import laa_maps_oracle as O
from tests import pd_cases as PC
from tests import pd_oracle as P

EPS = O.EPS
LU_GRAPHS = ("u8", "u12", "u16", "u30")


# ---------------------------------------------------------------------------------------------------------------- against the LU text
@pytest.mark.parametrize("pdmaxiter", [1, 2, 8])
@pytest.mark.parametrize("graph", LU_GRAPHS)
def test_restatement_against_the_lu_reference(graph, pdmaxiter):
    case = (graph, 1, 1.0, pdmaxiter)
    res, _ = PC.solved(case)
    x, traces = PC.lu_reference(case)
    d = PC.describe(res)
    gap = float(np.abs(res["x"] - x).max())
    print(f"[pd host] {graph} pdmaxiter={pdmaxiter}: |x - x_LU| = {gap:.3g}, steps (a) {[len(t['steps']) for t in d]} LU {[t['steps'] for t in traces]}")
    assert [len(t["steps"]) for t in d] == [t["steps"] for t in traces]
    assert res["steps"] == sum(t["steps"] for t in traces) and res["ill"] == res["stuck"] == 0
    assert all(t["ill"] == t["stuck"] == 0 for t in traces)
    assert np.all(res["x"][0] == 0)
    assert gap <= 1e-9


@pytest.mark.parametrize("graph", LU_GRAPHS)
def test_deep_exits_of_both_sides_are_printed(graph):
    """pdmaxiter = 64: the CG restatement and the LU restatement are expected to leave differently (module docstring); only printed."""
    case = (graph, 1, 1.0, 64)
    res, _ = PC.solved(case)
    _, traces = PC.lu_reference(case)
    d = PC.describe(res)
    print(f"[pd host] {graph} pdmaxiter=64: (a) " + ", ".join(f"{t['end']} {t['steps'][-1] if t['steps'] else 0}" for t in d) +
          " | LU " + ", ".join(f"{'ill' if t['ill'] else 'stuck' if t['stuck'] else 'maxiter'} after {t['steps']}" for t in traces))
    assert res["trace"].shape[0] >= 2


# ---------------------------------------------------------------------------------------------------------------- against (b)
def test_single_step_formulas_against_mpmath():
    case = ("u12", 1, 1.0, 8)
    n, ii, jj, _, _ = PC.case_inputs(case)
    _, seen = PC.solved(case, watch_steps=(1, 2, 5))
    worst = dict(pre=0.0, dir=0.0, resid=0.0)
    for step in (1, 2, 5):
        before, scal, after, _ = seen[(step, "pre")]
        b, mag = P.pre_b(before, scal["tau"])
        for k in b:
            r = O.few_ulp(after[k], after[k], b[k], mag[k])
            assert r["nonfinite_same"] and r["worst_a_ulp"] <= 16, (step, k, r)
            worst["pre"] = max(worst["pre"], r["worst_a_ulp"])
        before, scal, after, part = seen[(step, "dir")]
        b, mag = P.direction_b(before, ii, jj, scal["tau"])
        for k in b:
            r = O.few_ulp(after[k], after[k], b[k], mag[k])
            assert r["nonfinite_same"] and r["worst_a_ulp"] <= 32, (step, k, r)
            worst["dir"] = max(worst["dir"], r["worst_a_ulp"])
        # the minima: every candidate of the reference's rule (:325-330) recomputed from (a)'s direction, MATLAB's min
        mins = P.host_min(part)
        for c in range(3):
            m1, m2, q1, q2 = after["l1"][:, c], after["l2"][:, c], after["d1"][:, c], after["d2"][:, c]
            lam = np.concatenate([(-m1 / q1)[q1 < 0], (-m2 / q2)[q2 < 0], [np.inf]])
            assert mins[c] == np.nanmin(lam)
        for stage, trial in (("resid", False), ("resid_trial", True)):
            before, scal, _, part = seen[(step, stage)]
            tot, mags = P.resid_b(before, scal["tau"], scal["s"], trial)
            got = P.host_sum(part)
            terms = before["y"].shape[0] + n
            for c in range(3):
                if not scal["act"][c]:
                    assert got[c] == 0.0
                    continue
                err = float(abs(O.mp.mpf(float(got[c])) - tot[c]))
                allow = (terms + 8) * EPS * mags[c]
                worst["resid"] = max(worst["resid"], err / allow)
                assert err <= allow, (step, stage, c, err, allow)
    print(f"[pd host] (a) against (b): pre {worst['pre']:.3g} ulp, dir {worst['dir']:.3g} ulp, resid {worst['resid']:.3g} of its allowance")


def test_init_and_accept_against_the_reference_text():
    """k_pd_init and k_pd_accept restated against the same lines of tests/irls_oracle.py's l1decode_pd, evaluated in NumPy."""
    n, ii, jj, B, _ = PC.case_inputs(("u12", 1, 1.0, 8))
    st = P.blank(n, len(ii)); st["y"] = B.copy()
    ymax = P.host_max(P.absmax(st))
    assert np.array_equal(ymax, np.abs(B).max(axis=0))
    st = P.init(st, ymax)
    u = 0.95 * np.abs(B) + 0.10 * np.abs(B).max(axis=0)
    assert O.bit_equal(st["u"], u) and O.bit_equal(st["f1"], -B - u) and O.bit_equal(st["f2"], B - u) and O.bit_equal(st["l1"], -1 / (-B - u))
    A = IO.amatrix(np.stack([ii + 1, jj + 1]), n).toarray()
    atv = P.gather(n, P.csr(n, ii, jj), st["ev1"], None, 0)
    assert np.all(atv[0] == 0) and np.allclose(atv[1:], A.T @ (st["l1"] - st["l2"]), rtol=0, atol=1e-12 * np.abs(st["l1"]).max())
    dg = P.gather(n, P.csr(n, ii, jj), np.abs(st["ev1"]), None, 2)
    assert np.allclose(dg[1:], np.abs(A).T @ np.abs(st["ev1"]), rtol=1e-13)


# ---------------------------------------------------------------------------------------------------------------- the reductions
def test_partial_reductions_are_restated_thread_by_thread():
    """_fold / _tree against a literal per-thread loop at a size with a second grid-stride pass, NaNs among the data."""
    g = np.random.default_rng(3)
    m = P.SPAN + 300
    v = g.normal(size=(m, 1)) * 10.0 ** g.uniform(-3, 3, size=(m, 1))
    v[g.integers(0, m, 50)] = np.nan
    for op, init, pyop in ((np.add, 0.0, lambda a, b: a + b), (np.fmin, np.inf, lambda a, b: b if a != a else (a if b != b else min(a, b))),
                           (np.fmax, 0.0, lambda a, b: b if a != a else (a if b != b else max(a, b)))):
        part = P._tree(P._fold(np.full((P.SPAN, 1), init), [(v, None)], op), op)
        for b in (0, 1, 255):                                       # blocks 0 and 1 hold the second pass, block 255 one pass
            th = []
            for t in range(256):
                a = init
                for e in range(b * 256 + t, m, P.SPAN):
                    a = pyop(a, float(v[e, 0]))
                th.append(a)
            st = 128
            while st > 0:
                for t in range(st):
                    th[t] = pyop(th[t], th[t + st])
                st >>= 1
            assert O.bit_equal([th[0]], part[b]), (op, b)
    assert P.host_min(np.array([[np.nan], [np.inf]]))[0] == np.inf and np.isnan(P.host_max(np.array([[np.nan]])))[0] == False      # noqa: E712
    assert P.host_max(np.array([[np.nan], [2.0]]))[0] == 2.0
    cl = P.csr(5, [0, 0, 1, 3], [1, 4, 4, 4])
    assert cl[0].tolist() == [0, 2, 4, 4, 5, 8] and cl[1].tolist() == [0, 1, 0, 2, 3, 1, 2, 3] and cl[2].tolist() == [-1, -1, 1, -1, -1, 1, 1, 1]
    for name in ("u16", "k6"):
        n, ii, jj, _ = PC.edge_log_start(name, 0)
        C = P.csr(n, ii, jj)
        for vtx, row in enumerate(O.csr_rows(n, ii, jj)):
            assert [(int(C[1][t]), float(C[2][t])) for t in range(C[0][vtx], C[0][vtx + 1])] == [(e, s) for e, s in row]


# ---------------------------------------------------------------------------------------------------------------- the scalar rules
def test_scalar_rules_against_a_hand_worked_table():
    """pd_trial (:332-346), pd_goes_on (:287, :350), pd_step_length (:325-330), pd_gather_coef, pd_sdg / pd_tau (:280-281) on values
    worked by hand.  The sdg < tol arm and the 32-trial limit are reached by these rows whatever the search finds."""
    # rr, resnorm, s, backiter -> verdict, s after, backiter after, s tried.  sqrt(rr) <= (1 - 0.01 s) resnorm
    table = [
        ((0.25, 1.0, 0.5, 0), (P.ACCEPT, 0.25, 1, 0.5)),              # 0.5 <= 0.995
        ((1.0, 1.0, 0.5, 0), (P.AGAIN, 0.25, 1, 0.5)),                # 1 > 0.995
        ((0.990025, 1.0, 0.5, 3), (P.ACCEPT, 0.25, 4, 0.5)),          # sqrt = 0.995 == the bound: <= holds
        ((float("nan"), 1.0, 0.5, 0), (P.AGAIN, 0.25, 1, 0.5)),       # NaN compares false: never accepted
        ((0.25, float("nan"), 0.5, 5), (P.AGAIN, 0.25, 6, 0.5)),
        ((0.25, 1.0, 0.5, 31), (P.ACCEPT, 0.25, 32, 0.5)),            # the 32nd trial may still accept
        ((0.25, 1.0, 0.5, 32), (P.STUCK, 0.25, 33, 0.5)),             # the 33rd is stuck even where the decrease suffices
        ((1.0, 1.0, 2.0 ** -40, 32), (P.STUCK, 2.0 ** -41, 33, 2.0 ** -40)),
        ((0.0, 0.0, 1.0, 0), (P.ACCEPT, 0.5, 1, 1.0)),                # 0 <= 0
    ]
    assert math.sqrt(0.990025) == (1.0 - 0.01 * 0.5) * 1.0
    for args, want in table:
        got = P.pd_trial(*args)
        assert (got[0], float(got[1]), got[2], float(got[3])) == want, (args, got)
    # a coordinate that never suffices: trials 1 .. 32 say AGAIN, the 33rd STUCK, s halved 33 times
    s, k = 0.99, 0
    verdicts = []
    while True:
        v, s, k, _ = P.pd_trial(4.0, 1.0, s, k)
        verdicts.append(v)
        if v != P.AGAIN:
            break
    assert verdicts == [P.AGAIN] * 32 + [P.STUCK] and s == 0.99 * 2.0 ** -33
    tol = 2.0 ** -52
    goes = [((1.0, 0, 2), 1), ((1.0, 2, 2), 0), ((1.0, 3, 2), 0), ((tol, 0, 2), 1), ((np.nextafter(tol, 0), 0, 2), 0), ((0.0, 0, 2), 0),
            ((-1.0, 0, 2), 0), ((float("nan"), 0, 2), 1), ((float("nan"), 2, 2), 0), ((float("inf"), 1, 2), 1), ((1.0, 0, 0), 0)]
    assert P.TOL == tol
    for args, want in goes:
        assert P.pd_goes_on(*args) == want, args
    assert P.pd_step_length(np.inf, np.inf) == 0.99 and P.pd_step_length(0.5, np.inf) == 0.99 * 0.5 and P.pd_step_length(2.0, 0.25) == 0.99 * 0.25
    assert P.pd_step_length(np.nan, 0.5) == 0.99 * 0.5 and P.pd_step_length(np.nan, np.nan) == 0.99      # fmin skips NaN, as MATLAB's min
    assert P.pd_gather_coef(1, 4.0) == -0.25 and P.pd_gather_coef(0, 4.0) == 0.0 and P.pd_gather_coef(1, np.inf) == 0.0
    assert np.signbit(P.pd_gather_coef(1, np.inf)) and np.isnan(P.pd_gather_coef(1, np.nan))
    assert P.pd_sdg(-1.5, -2.5) == 4.0 and P.pd_tau(29.0, 4.0) == 145.0 and P.pd_tau(3.0, 0.0) == np.inf


# ---------------------------------------------------------------------------------------------------------------- the recorded cases
def test_recorded_cases_still_do_what_they_were_recorded_for():
    F = PC.FOUND
    assert set(F) == {"stuck_while_another_goes_on", "cg_breakdown", "tol", "three_trial_counts", "cg_cap"} and F["tol"] is None
    f = F["stuck_while_another_goes_on"]
    tr = PC.solved(f["case"])[0]["trace"]
    c, k = f["coordinate"], f["step"]
    assert tr[k, c, 0] == 1 and tr[k, c, 4] == P.STUCK and tr[k, c, 3] == 33 and tr[k + 1, c, 0] == 0
    assert sum(tr[k + 1, o, 0] for o in range(3) if o != c) >= 1
    f = F["cg_breakdown"]
    n, ii, jj, B, _ = PC.case_inputs(f["case"])
    res = PC.solved(f["case"])[0]; tr = res["trace"]
    c, k = f["coordinate"], f["step"]
    assert np.all(np.isfinite(B)) and tr[k, c, 0] == 1 and tr[k, c, 1] == 1 and tr[k, c, 3] == 0 and tr[k + 1, c, 0] == 0
    assert tr.shape[0] > k + 1 and tr[k + 1, :, 0].sum() >= 1 and np.all(np.isfinite(res["x"]))
    f = F["three_trial_counts"]
    tr = PC.solved(f["case"])[0]["trace"]
    assert tuple(int(t) for t in tr[f["step"], :, 3]) == f["trials"] and len(set(f["trials"])) == 3 and np.all(tr[f["step"], :, 4] == P.ACCEPT)
    f = F["cg_cap"]
    res = PC.solved(f["case"])[0]
    assert f["step"] in res["cap_steps"] and res["cg_unconverged"] == len(res["cap_steps"])
    for case in PC.SOLVER_CASES:
        d = PC.describe(PC.solved(case)[0])
        print(f"[pd host] {case}: " + ", ".join(f"{t['end']} {t['steps'][-1]}" for t in d))
        assert all(t["end"] in ("ill", "stuck") for t in d)                   # no coordinate reaches sdg < tol or step 64

"""CPU qualification of tests/exact_data_cases.py: what keeps tests/test_gpu_exact_data.py from passing vacuously.  No device.

Per case it states (run with -s) and asserts: that the v4 problems give S0 in {0, 1} bit for bit; which share of the clean / half-turn
cycles' cosines falls on either side of +-1 and exactly on it; that the restated CEMP parts are oracle/cemp_oracle.py's bits; how many
segments of the PGD cases hold tied weights and how many weights are exactly zero, and that the C oracle and the literal sort-and-scan
projection (oracle/desc_pgd_literal.py) agree there; that s0_enclosure contains NumPy's and the C oracle's value of every cycle and is
tight; and every MEASURED figure of the cases module."""
import numpy as np
import pytest

from oracle import desc_pgd_literal as lit
from oracle.cemp_oracle import cemp_oracle
from oracle.desc_pgd_literal import matlab_abs_acos
from tests import exact_data_cases as X


def _pgd_structure(oracle, name):
    mo = X.problem(*X.S0_CASES[name])
    nn, ii, jj, rij = X.marshalled(mo)
    st = oracle.build_structure(nn, ii, jj, seed=X.SEED, n_sample_min=X.NMIN)
    return mo, st, oracle.cycle_d(ii, jj, rij.reshape(-1, 9), st)


def _split(x, c):
    return float((x > c).mean()), float((x < c).mean()), float((x == c).mean())


# ---- v4: nothing to round ---------------------------------------------------------------------------------------------------------
def test_v4_s0_is_zero_or_one_bit_for_bit(oracle):
    for name in ("v4-40", "v4-120"):
        mo, st, S0 = _pgd_structure(oracle, name)
        assert np.array_equal(np.unique(S0), [0.0, 1.0]), name
        A, B, C, l, ejk, eki = X.pgd_cycles(mo, st)
        odd = (mo.corrupted[l].astype(int) + mo.corrupted[ejk] + mo.corrupted[eki]) > 0
        assert np.array_equal(X.cosines_f64(A, B, C), 1.0 - 2.0 * (S0 == 1.0))          # x is 1 or -1
        print("%s: %d cycles, %d consistent (S0 = 0), %d not (S0 = 1); %d hold a corrupted edge" % (name, S0.size, (S0 == 0).sum(), (S0 == 1).sum(), odd.sum()))
        assert (S0[~odd] == 0).all() and (S0 == 1).sum() > S0.size // 10
    kind, key = X.CEMP_CASES["v4"]
    assert np.array_equal(np.unique(X.cemp_cycles(kind, key).S0), [0.0, 1.0])
    for ns in X.CEMP_NSAMPLES:
        parts = X.cemp_parts(kind, key, ns, X.SEED)
        assert np.array_equal(np.unique(parts.S0), [0.0, 1.0])
        S = X.cemp_variants(kind, key, ns, X.SEED)[0]
        allzero = parts.pos & (parts.S0 == 0).all(axis=0)
        print("v4 nsample %d: %d of %d edges sampled consistent cycles only; after six rounds %d edges at exactly 0, %d at exactly 1"
              % (ns, allzero.sum(), allzero.size, (S == 0).sum(), (S == 1).sum()))
        assert allzero.sum() >= 5 and (S[allzero] == 0.0).all()


# ---- clean and half-turn: the cosines straddle the branch points ------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in X.S0_CASES if not k.startswith("v4")])
def test_cosines_fall_on_both_sides_of_the_branch_point(oracle, name):
    mo, st, S0 = _pgd_structure(oracle, name)
    A, B, C, l, ejk, eki = X.pgd_cycles(mo, st)
    bad = mo.corrupted[l].astype(int) + mo.corrupted[ejk] + mo.corrupted[eki]
    c, sel = (1.0, bad == 0) if name.startswith("clean") else (-1.0, bad == 1)
    above, below, on = _split(X.cosines_f64(A, B, C)[sel], c)
    print("%s: %d of %d cycles %s; cosine above %+g: %.1f %%, below: %.1f %%, exactly on it: %.1f %%"
          % (name, sel.sum(), sel.size, "consistent" if c > 0 else "hold one half-turn edge", c, 100 * above, 100 * below, 100 * on))
    assert above >= 0.1 and below >= 0.1 and on > 0


@pytest.mark.parametrize("name", ["clean", "half"])
def test_cemp_cosines_fall_on_both_sides_of_the_branch_point(name):
    kind, key = X.CEMP_CASES[name]
    mo, cy = X.problem(kind, key), X.cemp_cycles(kind, key)
    bad = mo.corrupted[cy.l].astype(int) + mo.corrupted[cy.ejk] + mo.corrupted[cy.eki]
    c, sel = (1.0, bad == 0) if name == "clean" else (-1.0, bad == 1)
    above, below, on = _split(cy.x64[sel], c)
    print("CEMP %s: %d of %d distinct cycles; cosine above %+g: %.1f %%, below: %.1f %%, exactly on it: %.1f %%"
          % (name, sel.sum(), sel.size, c, 100 * above, 100 * below, 100 * on))
    assert above >= 0.1 and below >= 0.1 and on > 0


# ---- the restated CEMP parts are the oracle's --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.CEMP_CASES))
def test_cemp_parts_give_the_oracle_bits(name):
    """cemp_rounds on cemp_parts' S0Mat against oracle/cemp_oracle.py: the initial means and six rounds, the same bits (the long
    nsample = 300 through the rounds only: the oracle takes seconds there)."""
    kind, key = X.CEMP_CASES[name]
    mo = X.problem(kind, key)
    for ns in X.CEMP_NSAMPLES:
        parts = X.cemp_parts(kind, key, ns, X.SEED)
        for rounds in ((0, 6) if ns <= 70 else (6,)):
            assert np.array_equal(X.cemp_rounds(parts.S0, parts, rounds), cemp_oracle(mo.Ind, mo.RijMat, rounds, X.BETA, ns, seed=X.SEED)), (ns, rounds)
        ref = X.cemp_variants(kind, key, ns, X.SEED)[0]
        cor = mo.corrupted & parts.pos
        print("CEMP %s nsample %d: clean edges at most %.3g, corrupted edges at least %.3g" % (name, ns, ref[~mo.corrupted & parts.pos].max(), ref[cor].min()))


# ---- PGD on ties ----------------------------------------------------------------------------------------------------------------
def _gradient(rule):
    kw = X.PGD_RULES[rule]
    return lit.ConstantStepSize(kw["lr"]) if kw["step_kind"] == 0 else lit.HybridGradient(kw["lr"], kw["beta1"], kw["beta2"], kw["decay_interval"])


@pytest.mark.parametrize("rule", list(X.PGD_RULES))
@pytest.mark.parametrize("pname", list(X.PGD_PROBLEMS))
def test_pgd_tie_cases_qualify(oracle, pname, rule):
    """`At least half of the segments hold a tied pair among their positive weights` is asserted where it holds: with q = 0 at both run
    lengths, and on the n = 120, q = 0.2 problem after the first projection (every rule) and at the end of the lr = 0.5 run.  It does not
    hold, for any of the model seeds 1-8 tried besides 11, at the end of a run at lr = 0.01 or with Adam (the groups dissolve within three
    iterations: q = 0.2 gives every cycle its own history) nor on the n = 40, q = 0.2 problem (a tenth of the segments); those cases
    state their counts and keep the rest of the qualification.  The literal restatement is dense in n: it runs on the n = 40 problems."""
    tol = X.PGD_TOL[rule]
    for iters in X.PGD_ITERS:
        (nn, ii, jj, rij), st, S0, ref, _ = X.pgd_reference(pname, rule, iters)
        w = ref["w"]
        tied, zeros = X.tied_segments(st, w), int((w == 0).sum())
        print("%s %s %d iterations: stopped at %d; %d of %d segments hold tied positive weights, %d of %d weights exactly 0, %d distinct S_vec values"
              % (pname, rule, iters, ref["iters_run"], tied, st["m_pos"], zeros, w.size, np.unique(ref["S_vec"]).size))
        assert np.array_equal(np.unique(S0), [0.0, 1.0]) or pname == "q0"
        if pname == "q0" or (pname == "q0.2-120" and (iters == 1 or rule == "lr0.5")):
            assert 2 * tied >= st["m_pos"], (iters, tied)
        if rule == "lr0.5" and pname != "q0" and iters == 100:
            assert zeros > w.size // 4
        if pname == "q0":                                   # every cycle consistent: S0 = 0, objective 0 from the first iteration on
            assert not S0.any() and not ref["obj"].any() and not ref["S_vec"].any()
            assert ref["iters_run"] == min(iters, X.PATIENCE + 1)
        if nn <= 40:
            mo = X.problem(*X.PGD_PROBLEMS[pname])
            S, state = lit.desc_pgd_literal(mo.Ind, mo.RijMat, iters, _gradient(rule), sampler=oracle.keyed_sampler(X.SEED), return_state=True)
            d = max(float(np.abs(S - ref["S_vec"]).max()), float(np.abs(state["wijk"] - w).max()))
            print("    literal sort-and-scan against the C oracle: %.3g (allowed %.3g), iterations %d / %d" % (d, tol / 16, state["iters_run"], ref["iters_run"]))
            assert state["iters_run"] == ref["iters_run"] and d <= tol / 16


# ---- the enclosure --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in X.S0_CASES if not k.startswith("v4")])
def test_enclosure_contains_both_f64_values_and_is_tight(oracle, name):
    mo, st, S0 = _pgd_structure(oracle, name)
    A, B, C, l, ejk, eki = X.pgd_cycles(mo, st)
    x = X.cosines_f64(A, B, C)
    lo, hi = X.s0_enclosure(A, B, C)
    for who, v in (("NumPy", matlab_abs_acos(x) / np.pi), ("C oracle", S0)):
        pos = X.position(v, lo, hi)
        print("%s %s: worst position in the enclosure %.3g" % (name, who, pos.min()))
        assert np.isfinite(v).all() and pos.min() >= 0
    width = hi - lo
    near = np.abs(np.abs(x) - 1) < 1e-9
    # away from +-1 the width is 2 dx |f'(x)| and the libm margin: f' = 1 / (pi sqrt(1 - x^2)), dx <= (28 u 3 sqrt(3) + 4 u) / 2
    generic = np.abs(x) < 0.9
    bound = 2 * (28 * X.U * 3 * 3 ** 0.5 + 4 * X.U) / 2 / (np.pi * np.sqrt(1 - 0.9 ** 2)) + 2 * X.LIBM + 4 * X.U
    print("%s: width at most %.3g on the %d cycles within 1e-9 of +-1, at most %.3g (%.0f ulp of 1) on the %d with |x| < 0.9 (bound %.3g)"
          % (name, width[near].max(), near.sum(), width[generic].max(), width[generic].max() / 2.0 ** -52, generic.sum(), bound))
    assert width[near].max() < 1e-7 and width[generic].max() <= bound


def test_enclosure_of_cemp_cycles_contains_the_oracle():
    for name in ("clean", "half"):
        cy = X.cemp_cycles(*X.CEMP_CASES[name])
        assert X.position(cy.S0, cy.lo, cy.hi).min() >= 0 and X.position(cy.S0x, cy.lo, cy.hi).min() >= 0
        assert (cy.hi - cy.lo)[np.abs(np.abs(cy.x64) - 1) < 1e-9].max() < 1e-7


def test_enclosure_at_chosen_points():
    """One cycle each: the identity (x = 1 exactly: [0, sqrt(2 dx) / pi]), a quarter turn (x = 0, well conditioned: a few ulps around
    1/2), a half turn (x = -1 exactly: holds 1 and reaches past it on the hypot side)."""
    I = np.eye(3)[None]
    q = np.array([[[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]])
    h = np.diag([1.0, -1, -1])[None]
    lo, hi = X.s0_enclosure(I, I, I)
    assert lo[0] == 0.0 and 0 < hi[0] < 4e-8
    lo, hi = X.s0_enclosure(q, I, I)
    assert lo[0] < 0.5 < hi[0] and hi[0] - lo[0] < 64 * X.U
    lo, hi = X.s0_enclosure(h, I, I)
    assert lo[0] < 1.0 < hi[0] and hi[0] - lo[0] < 8e-8 and hi[0] - 1 < 1e-14          # hypot(pi, t) - pi = t^2 / (2 pi): flat beyond -1
    mlo, mhi = X.mean_enclosure(np.array([[0.0, 0.5]]).T, np.array([[0.0, 0.5]]).T, axis=0)
    assert mlo[0] < 0.25 < mhi[0] and mhi[0] - mlo[0] < 8 * X.U


# ---- the measured tolerances ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clean", "half"])
def test_measured_cemp(name):
    kind, key = X.CEMP_CASES[name]
    worst = 0.0
    for ns in X.CEMP_NSAMPLES:
        ref, ext, far = X.cemp_variants(kind, key, ns, X.SEED)
        a, b = float(np.abs(ref - ext).max()), float(np.abs(ref - far).max())
        print("CEMP %s nsample %d: (a) oracle against extended-precision traces %.3g, (b) against the far ends of the enclosures %.3g" % (name, ns, a, b))
        worst = max(worst, a, b)
    print("CEMP %s: measured %.3g, MEASURED %.3g, TOL %.3g" % (name, worst, X.CEMP_MEASURED[name], X.CEMP_TOL[name]))
    assert X.CEMP_MEASURED[name] / 2 <= worst <= X.CEMP_MEASURED[name]


@pytest.mark.parametrize("case", list(X.E2E_CASES))
def test_measured_end_to_end(oracle, case):
    mo = X.problem(*X.E2E_CASES[case])
    for call in X.E2E_CALLS:
        ref = X.e2e_oracle(call, case)
        err, R = X.aligned_error(ref["R"], mo.R_orig), ref["R"]
        print("%s %s: the oracle's aligned error %.3g, MEASURED %.3g, TOL %.3g; SO(3) defect %.2g; %s"
              % (case, call, err, X.E2E_MEASURED[case][call], X.E2E_TOL[case][call], X.so3_defect(R), {k: v for k, v in ref.items() if k not in ("R", "S")}))
        assert np.isfinite(R).all() and err <= X.E2E_MEASURED[case][call]
    assert X.e2e_oracle("DESC", case)["iters"] == 1

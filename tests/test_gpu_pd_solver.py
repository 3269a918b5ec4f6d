"""pd_solve (desc_amd/csrc/irls.hip), the host loop around the primal-dual kernels, through desc_test_irls_pd_solve against restatement
(a) of tests/pd_oracle.py: x, the final u, lamu1, lamu2, Ax, Atv and every field of the per-step trace bit-equal, every counter equal.
The trace is one record per step and coordinate: takes part, the CG's bad, the first trial step, the number of trials, the verdict, and
sdg, tau, resnorm after the step; so every decision of the loop (run / search / accept per coordinate) is compared, not only its result.

Case -> line reached (irls.hip, pd_solve)
  u8 / u12 / u16 / u30, pdmaxiter 0              the start alone: pd_goes_on's `pditer >= pdmaxiter` arm before any step; x = 0
  the same, pdmaxiter 1, 2, 8                    the loop as the L1 stage runs it (2) and past it; all coordinates together
  u8 seed 1, 1e-3 B, pdmaxiter 64                "stuck": pd_trial's 32-trial limit, coordinate 0 in step 19 while 1 and 2 go on to 26
                                                 and 33: run[] / search[] / accept[] with the coordinates apart, k_pd_accept moving some
                                                 coordinates while another stands, the act masks of every kernel
  u8 seed 0, B, pdmaxiter 64                     "ill" by a CG breakdown on finite data (coordinates 0, 1 in step 11, 2 in step 13); step 12
                                                 at the CG cap (cg_unconverged)
  u8 seed 0, 1e-3 B, pdmaxiter 64                28, 1 and 4 backtracking trials in one step: search[] ends per coordinate
  planar                                         two all-zero coordinates: NaN from the start, "ill" at the first solve, no step counted,
                                                 x = 0 exactly (the header's documented deviation from the reference's "stuck")
  sdg < tol                                      reached by no case of the search space (tests/test_pd_host.py): the rule alone is
                                                 tested there

Mutation note (two scratch builds, never committed, each run on an MI355X against this file, tests/test_gpu_pd_kernels.py and
tests/test_gpu_irls.py):
  k_pd_accept ignoring act (every coordinate moved by its s in every launch)
      fails here: test_solver_is_bit_equal_to_the_restatement in 15 of its 19 cases (pdmaxiter 0 included: the launch that only forms
      the start's dot products now moves the state by 0 * direction with the direction arrays not yet written),
      test_the_recorded_exits_are_taken_on_the_device, test_planar_zero_coordinates; in the kernel file test_act_masks[accept].
      tests/test_gpu_irls.py does NOT pass under it either: 5 of its tests fail (test_two_runs_are_bitwise_equal, test_c4[GM],
      test_rinit_sigma_and_max_iterations and two L12 cases), through that same start launch; the others pass.
  on "stuck" the host loop clears run[(c + 1) % 3] instead of run[c] (the scratch build also bounds the loop by pdmaxiter: the
  coordinate left running would otherwise never end)
      fails here: test_solver_is_bit_equal_to_the_restatement on both cases that reach "stuck" (u8 seed 0 and seed 1 at 1e-3 B) and
      test_the_recorded_exits_are_taken_on_the_device; everything else passes.  tests/test_gpu_irls.py passes whole: none of its
      graphs reaches the 32-trial limit.

Measured on an MI355X: every comparison bit-equal -- 19 parametrised cases (up to 33 steps, 78 coordinate steps, 33 trials in a step, one
Newton solve at the CG cap of 360 steps), planar at pdmaxiter 2 and 8 (x(:, 1:2) = +0 exactly, ill = 2, steps = pdmaxiter; z bit-equal
both to a run with z's data in all three coordinates and to one with the 16-node problem's x and y data), two runs the same bits.  The
slowest case takes 0.2 s.  Every test prints what it measured (run with -s)."""
import numpy as np
import pytest

from tests import irls_batch_cases as BC
from tests import laa_maps_cases as K
from tests import laa_maps_oracle as O
from tests import pd_cases as PC
from tests import pd_oracle as P

pytestmark = pytest.mark.gpu

ARRAYS = ("x", "u", "l1", "l2", "Ax", "Atv")
COUNTERS = ("steps", "ill", "stuck", "solves", "cg_total", "cg_unconverged")
CASES = [(g, 1, 1.0, it) for g in ("u8", "u12", "u16", "u30") for it in (0, 1, 2, 8)] + PC.SOLVER_CASES


def device_solve(lib, n, ii, jj, B, pdmaxiter):
    dp = lib.DeviceProblem(lib.ProblemArrays(n, np.asarray(ii, dtype=np.int32), np.asarray(jj, dtype=np.int32), K.identity_rij(len(ii))))
    return lib.hook_pd_solve(dp, B, pdmaxiter)


def assert_same(tag, got, want):
    for k in COUNTERS:
        assert got[k] == want[k], f"{tag}: {k} {got[k]} != {want[k]}"
    assert got["trace"].shape == want["trace"].shape, f"{tag}: {got['trace'].shape[0]} trace records, (a) has {want['trace'].shape[0]}"
    for f, name in enumerate(P_TRACE):
        assert O.bit_equal(got["trace"][:, :, f], want["trace"][:, :, f]), f"{tag}: trace field {name} differs at {np.argwhere(got['trace'][:, :, f] != want['trace'][:, :, f])[:4].tolist()}"
    for k in ARRAYS:
        assert O.bit_equal(got[k], want[k]), f"{tag}: {k} differs from (a)"


P_TRACE = ("part", "bad", "s", "trials", "verdict", "sdg", "tau", "resnorm")


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-seed{c[1]}-x{c[2]:g}-it{c[3]}")
def test_solver_is_bit_equal_to_the_restatement(lib, case):
    n, ii, jj, B, pdmaxiter = PC.case_inputs(case)
    want, _ = PC.solved(case)
    got = device_solve(lib, n, ii, jj, B, pdmaxiter)
    d = PC.describe(want)
    print(f"[pd solver] {case}: steps {got['steps']} ill {got['ill']} stuck {got['stuck']} solves {got['solves']} CG {got['cg_total']} "
          f"(at the cap: {got['cg_unconverged']}); ends " + ", ".join(f"{t['end']} {t['steps'][-1] if t['steps'] else 0}" for t in d) +
          f"; trials up to {int(got['trace'][:, :, 3].max())}")
    assert_same(str(case), got, want)
    if pdmaxiter == 0:
        assert np.all(got["x"] == 0) and got["trace"].shape[0] == 1 and got["solves"] == 0
    assert np.all(got["x"][0] == 0) and np.all(got["Atv"][0] == 0)


def test_the_recorded_exits_are_taken_on_the_device(lib):
    """What each case of pd_cases.FOUND was recorded for, read from the device's own trace."""
    F = PC.FOUND
    tr = {}
    for case in PC.SOLVER_CASES:
        n, ii, jj, B, pdmaxiter = PC.case_inputs(case)
        tr[case] = device_solve(lib, n, ii, jj, B, pdmaxiter)
    f = F["stuck_while_another_goes_on"]; t = tr[f["case"]]["trace"]
    assert t[f["step"], f["coordinate"], 4] == P.STUCK and t[f["step"], f["coordinate"], 3] == 33 and t[f["step"] + 1, f["coordinate"], 0] == 0
    assert t[f["step"] + 1, :, 0].sum() == 2 and tr[f["case"]]["stuck"] == 3
    f = F["cg_breakdown"]; t = tr[f["case"]]["trace"]
    assert t[f["step"], f["coordinate"], 1] == 1 and t[f["step"] + 1, :, 0].sum() >= 1 and np.all(np.isfinite(tr[f["case"]]["x"]))
    f = F["three_trial_counts"]; t = tr[f["case"]]["trace"]
    assert tuple(int(v) for v in t[f["step"], :, 3]) == f["trials"]
    f = F["cg_cap"]
    assert tr[f["case"]]["cg_unconverged"] >= 1
    print("[pd solver] recorded exits taken on the device: stuck apart, CG breakdown on finite data, trials " + str(F["three_trial_counts"]["trials"]) +
          f", CG cap x{tr[f['case']]['cg_unconverged']}")


def test_planar_zero_coordinates(lib):
    """planar of tests/irls_batch_cases.py: the x and y coordinates of B are exactly zero.  They return x = 0 exactly with ill = 1 each
    and no step counted; the z coordinate has the bits of a run in which the other two coordinates hold ordinary data.  (The three
    Newton systems share one CG, which runs until the slowest coordinate of the test has converged: z's bits are those of a run whose
    other coordinates need no more CG steps than z does: compared with z's own data in all three, and with the 16-node problem's x
    and y data, where restatement (a) gives z the same bits as well.)"""
    Ind, Rij = BC.planar()
    order = np.lexsort((Ind[:, 1], Ind[:, 0]))
    Ind, Rij = Ind[order], Rij[:, :, order]
    n = int(Ind.max()); ii, jj = Ind[:, 0] - 1, Ind[:, 1] - 1
    from oracle.refine_oracle import R2Q
    from tests import irls_oracle as IO
    QQ = R2Q(IO.project(np.transpose(Rij, (1, 0, 2)))[0])
    I = np.stack([ii + 1, jj + 1])
    B = IO.edge_log(I, IO.tree_start(I, QQ, n)[0], QQ)
    assert np.all(B[:, :2] == 0) and np.count_nonzero(B[:, 2]) == len(ii) - (n - 1)          # the tree's own edges have B = 0
    n16, i16, j16, B16 = PC.edge_log_start("u16", 1)                              # planar's graph is this one
    assert n16 == n and np.array_equal(i16, ii) and np.array_equal(j16, jj)
    for it in (2, 8):
        got = device_solve(lib, n, ii, jj, B, it)
        want = P.solve(n, ii, jj, B, it)
        assert_same(f"planar it={it}", got, want)
        assert np.all(got["x"][:, :2] == 0) and not np.signbit(got["x"][:, :2]).any()
        assert got["ill"] == 2 and got["stuck"] == 0 and got["steps"] == it and got["trace"][1, :, 1].tolist() == [1, 1, 0]
        assert np.all(got["trace"][2:, :2, 0] == 0)
        full = device_solve(lib, n, ii, jj, np.repeat(B[:, 2:3], 3, axis=1), it)
        assert full["ill"] == 0 and full["steps"] == 3 * it
        for k in ARRAYS:
            assert O.bit_equal(got[k][:, 2], full[k][:, 2]), k
        assert O.bit_equal(got["trace"][:, 2], full["trace"][:, 2])
        mixed = device_solve(lib, n, ii, jj, np.stack([B16[:, 0], B16[:, 1], B[:, 2]], axis=1), it)
        assert mixed["ill"] == 0
        for k in ARRAYS:
            assert O.bit_equal(got[k][:, 2], mixed[k][:, 2]), k
        assert O.bit_equal(got["trace"][:, 2], mixed["trace"][:, 2])
        print(f"[pd solver] planar pdmaxiter={it}: x(:, 1:2) = 0 exactly, ill 2, steps {got['steps']}; z bit-equal to the run with z's data in all three coordinates")


def test_two_runs_give_the_same_bits(lib):
    case = PC.FOUND["stuck_while_another_goes_on"]["case"]
    n, ii, jj, B, pdmaxiter = PC.case_inputs(case)
    a, b = device_solve(lib, n, ii, jj, B, pdmaxiter), device_solve(lib, n, ii, jj, B, pdmaxiter)
    assert_same("rerun", a, b)
    print(f"[pd solver] two runs of {case}: {a['trace'].shape[0]} trace records, all arrays and counters the same bits")


def test_bad_arguments_are_refused_before_any_device_work(lib):
    L = lib.load()
    n, ii, jj = K.path_graph(4)
    dp = lib.DeviceProblem(lib.ProblemArrays(n, ii, jj, K.identity_rij(len(ii))))
    m, h = dp.m, dp.handle
    d = np.zeros(17 * 3 * m + 6 * 256); p = lib.ptr(d, lib.F64P)
    i32 = np.zeros(8, dtype=np.int32); pi = lib.ptr(i32, lib.I32P)
    calls = [
        L.desc_test_irls_pd_stage(None, 0, p, p, p, pi, m, n, p, p, p), L.desc_test_irls_pd_stage(h, 0, None, p, p, pi, m, n, p, p, p),
        L.desc_test_irls_pd_stage(h, 0, p, p, p, None, m, n, p, p, p), L.desc_test_irls_pd_stage(h, 0, p, p, p, pi, m, n, None, p, p),
        L.desc_test_irls_pd_stage(h, 0, p, p, p, pi, m, n, p, None, p), L.desc_test_irls_pd_stage(h, 0, p, p, p, pi, m, n, p, p, None),
        L.desc_test_irls_pd_stage(h, 0, p, p, p, pi, m + 1, n, p, p, p), L.desc_test_irls_pd_stage(h, 0, p, p, p, pi, m, n + 1, p, p, p),
        L.desc_test_irls_pd_stage(h, -1, p, p, p, pi, m, n, p, p, p), L.desc_test_irls_pd_stage(h, len(lib.PD_STAGES), p, p, p, pi, m, n, p, p, p),
        L.desc_test_irls_pd_solve(None, p, m, n, 2, p, p, pi, p, 3, pi), L.desc_test_irls_pd_solve(h, None, m, n, 2, p, p, pi, p, 3, pi),
        L.desc_test_irls_pd_solve(h, p, m, n, 2, None, p, pi, p, 3, pi), L.desc_test_irls_pd_solve(h, p, m, n, 2, p, p, pi, p, 3, None),
        L.desc_test_irls_pd_solve(h, p, m - 1, n, 2, p, p, pi, p, 3, pi), L.desc_test_irls_pd_solve(h, p, m, n - 1, 2, p, p, pi, p, 3, pi),
        L.desc_test_irls_pd_solve(h, p, m, n, -1, p, p, pi, p, 3, pi),
    ]
    assert all(rc == lib.ERR_INVALID for rc in calls), calls
    assert np.all(d == 0)

"""GPU tests of the batched solver (desc_pgd_batch_*, DESC_PGD_batch): every problem of a batch against the CPU oracle run on that
problem ALONE, with the tolerances of tests/test_gpu_parity.py (check), and bitwise against itself in other batches.

Figures quoted in the docstrings (longest segments, n_sample, oracle iters_run) are asserted from the oracle, sampling seed 1."""
import numpy as np
import pytest

from tests.helpers import assert_structure_equal, c_params, make_problem, oracle_reference

pytestmark = pytest.mark.gpu
TOL = 1e-10
SEED = 1
MIXED = [(12, 0.6, 9), (40, 0.5, 10), (90, 0.5, 8), (150, 0.95, 6), (200, 0.5, 4)]      # (n, p, model seed)


def check(out, ref, s0, S0, tol=TOL):
    """tests/test_gpu_parity.py: check, for vectors that may be empty (a problem without a triangle)."""
    mx = lambda a, b: float(np.abs(a - b).max()) if a.size else 0.0
    assert s0.shape == S0.shape and mx(s0, S0) <= 1e-14
    assert out["iters_run"] == ref["iters_run"]
    assert out["S_vec"].shape == ref["S_vec"].shape and mx(out["S_vec"], ref["S_vec"]) <= tol
    assert out["w"].shape == ref["w"].shape and mx(out["w"], ref["w"]) <= tol
    assert out["obj"].shape == ref["obj"].shape and np.allclose(out["obj"], ref["obj"], rtol=1e-12, atol=1e-9)
    assert out["avg"].shape == ref["avg"].shape and np.allclose(out["avg"], ref["avg"], rtol=1e-9, atol=1e-14)


def uniform(n, p, seed, q=0.2, sigma=0.1):
    mo, nn, ii, jj, rij = make_problem("uniform", n=n, p=p, q=q, sigma=sigma, seed=seed)
    return dict(mo=mo, n=nn, ii=ii, jj=jj, rij=rij)


def path_graph(n=8):
    ii = np.arange(n - 1, dtype=np.int32)
    return dict(mo=None, n=n, ii=ii, jj=ii + 1, rij=np.tile(np.eye(3).reshape(-1), n - 1))


def run_batch(lib, probs, p, seeds=None, want_w=True, adam=None, structures=False):
    arrs = [lib.ProblemArrays(q["n"], q["ii"], q["jj"], q["rij"]) for q in probs]
    b = lib.Batch(arrs, p, seeds)
    try:
        sts = [b.structure(k) for k in range(b.count)] if structures else None
        s0 = b.s0()
        outs, timings = b.run(p, want_w=want_w, adam=adam)
    finally:
        b.destroy()
    return sts, s0, outs


def reference(oracle, q, seed, iters, **step):
    return oracle_reference(oracle, q["n"], q["ii"], q["jj"], q["rij"], seed=seed, iters=iters, **step)


@pytest.fixture(scope="module")
def mixed(oracle):
    """The batch of case 1 and its oracle runs (100 iterations, lr = 0.01), computed once."""
    probs = [uniform(n, p, s) for n, p, s in MIXED]
    refs = [reference(oracle, q, SEED, 100, lr=0.01) for q in probs]
    return probs, refs


@pytest.fixture(scope="module")
def mixed_gpu(lib, mixed):
    probs, refs = mixed
    return run_batch(lib, probs, c_params(100, lr=0.01, seed=SEED), structures=True)


def test_mixed_batch_all_lane_group_widths(mixed, mixed_gpu):
    """Longest segments 5, 17, 30, 34, 30: lane groups of 16, 32 and 64 in one launch; n_sample = 34 for the fourth problem."""
    probs, refs = mixed
    sts, s0, outs = mixed_gpu
    assert [int(np.diff(st["cum_ind"]).max()) for st, _, _ in refs] == [5, 17, 30, 34, 30]
    assert refs[3][0]["n_sample"] == 34
    for (st, S0, ref), got_st, got_s0, out in zip(refs, sts, s0, outs):
        assert_structure_equal(got_st, st)
        assert out["n_sample"] == st["n_sample"]
        check(out, ref, got_s0, S0)
        assert out["iters_run"] == 100 and out["t_end"] == 100


@pytest.fixture(scope="module")
def early(oracle):
    probs = [uniform(40, 0.5, 10, q=0.1, sigma=0.0), uniform(12, 0.6, 9), uniform(90, 0.5, 8, q=0.3), uniform(200, 0.5, 4), path_graph(8)]
    refs = [reference(oracle, q, SEED, 400, lr=1.0, patience=5, stop_tol=1e-3) for q in probs]
    return probs, refs


@pytest.mark.parametrize("check_every", [0, 3])
def test_per_problem_early_stop(lib, early, check_every):
    """Five problems that stop at five different iterations (oracle: 12, 26, 393, 155 and, for the triangle-free path graph,
    patience + 1 = 6): a frozen problem's state, the parity of the buffer that holds it and the length of its traces."""
    probs, refs = early
    its = [ref["iters_run"] for _, _, ref in refs]
    assert its == [12, 26, 393, 155, 6] and len(set(its)) == 5
    p = c_params(400, lr=1.0, seed=SEED, patience=5, stop_tol=1e-3, check_every=check_every)
    sts, s0, outs = run_batch(lib, probs, p, structures=True)
    for k, ((st, S0, ref), out) in enumerate(zip(refs, outs)):
        assert_structure_equal(sts[k], st)
        check(out, ref, s0[k], S0)
        assert out["t_end"] == ref["iters_run"]
    assert np.array_equal(outs[4]["S_vec"], np.ones(7)) and outs[4]["w"].size == 0 and not outs[4]["obj"].any()


def _same_bits(a, b):
    for key in ("S_vec", "w", "obj", "avg"):
        assert np.array_equal(a[key], b[key]), key
    assert a["iters_run"] == b["iters_run"]


def test_composition_independence_bitwise(lib, mixed, mixed_gpu):
    """The batch as given, reversed, and every problem as a batch of one: the same bits per problem.  Per-problem seeds equal the
    same problems run alone with those seeds."""
    probs, _ = mixed
    _, _, outs = mixed_gpu
    p = c_params(100, lr=0.01, seed=SEED)
    _, _, rev = run_batch(lib, probs[::-1], p)
    for k in range(len(probs)):
        _same_bits(outs[k], rev[len(probs) - 1 - k])
        _, _, alone = run_batch(lib, [probs[k]], p)
        _same_bits(outs[k], alone[0])
    seeds = [7, 1, 123456789012, 0, 5]
    p30 = c_params(30, lr=0.01, seed=99)
    sts, _, seeded = run_batch(lib, probs, p30, seeds=seeds, structures=True)
    for k, sd in enumerate(seeds):
        q = c_params(30, lr=0.01, seed=sd)
        st1, _, alone = run_batch(lib, [probs[k]], q, structures=True)
        assert_structure_equal(sts[k], st1[0])
        _same_bits(seeded[k], alone[0])
    assert not np.array_equal(sts[3]["k"], mixed_gpu[0][3]["k"])                         # seed 0 samples other cycles than seed 1


def test_more_problems_than_compute_units(lib, oracle):
    """300 problems of 12 nodes, some of them partly triangle-free: the workgroup table past one workgroup per CU."""
    probs = []
    for s in range(300):
        try:
            q = uniform(12, 0.6, s)
        except Exception:                       # the generator refuses degenerate graphs
            continue
        if q["ii"].shape[0]:
            probs.append(q)
    assert len(probs) >= 290
    refs = [reference(oracle, q, SEED, 30, lr=0.01) for q in probs]
    sts, s0, outs = run_batch(lib, probs, c_params(30, lr=0.01, seed=SEED), structures=True)
    assert len(outs) == len(probs)
    for k, ((st, S0, ref), out) in enumerate(zip(refs, outs)):
        assert_structure_equal(sts[k], st)
        check(out, ref, s0[k], S0)


STEP_RULES = dict(large_lr=dict(step_kind=0, lr=1.0),
                  piecewise=dict(step_kind=1, lr=0.05, decay_interval=7, t0=3),
                  hybrid_adam=dict(step_kind=2, lr=0.001, beta1=0.9, beta2=0.999, decay_interval=10),
                  hybrid_plain=dict(step_kind=2, lr=0.0005, decay_interval=10, hybrid_strategy=1, t0=4))


@pytest.fixture(scope="module")
def two():
    return [uniform(90, 0.5, 8, q=0.3), uniform(40, 0.5, 10)]


@pytest.mark.parametrize("kind", sorted(STEP_RULES))
def test_step_rules(lib, oracle, two, kind):
    """The four parameter sets of test_step_plugins on a batch of two, 40 iterations."""
    kw = STEP_RULES[kind]
    tol = 1e-9 if kind == "hybrid_adam" else TOL        # Adam divides by sqrt(v) + 1e-8: rounding differences are amplified where v ~ 0
    refs, states = [], []
    for q in two:
        st = oracle.build_structure(q["n"], q["ii"], q["jj"], seed=5)
        S0 = oracle.cycle_d(q["ii"], q["jj"], q["rij"].reshape(-1, 9), st)
        am, av = np.zeros(st["m_cycle"]), np.zeros(st["m_cycle"])
        ref = oracle.pgd_run(st, S0, 40, adam_m=am, adam_v=av, **kw) if kind == "hybrid_adam" else oracle.pgd_run(st, S0, 40, **kw)
        refs.append((st, S0, ref)); states.append((am, av))
    mc = sum(st["m_cycle"] for st, _, _ in refs)
    adam = (np.zeros(mc), np.zeros(mc)) if kind == "hybrid_adam" else None
    _, s0, outs = run_batch(lib, two, c_params(40, seed=5, **kw), adam=adam)
    for (st, S0, ref), out, got_s0, (am, av) in zip(refs, outs, s0, states):
        check(out, ref, got_s0, S0, tol=tol)
        assert out["t_end"] == kw.get("t0", 0) + ref["iters_run"]
        if kind == "hybrid_adam":
            assert np.abs(out["adam_m"] - am).max() <= 1e-9 and np.abs(out["adam_v"] - av).max() <= 1e-9 and np.abs(av).max() > 0
    if kind != "hybrid_adam":
        return
    # the moments go in again: 10 more iterations from t0 = 40 (handle-object semantics of HybridGradient)
    cont = dict(kw, t0=40)
    _, _, outs2 = run_batch(lib, two, c_params(10, seed=5, **cont), adam=adam)
    for (st, S0, _), out, (am, av) in zip(refs, outs2, states):
        # the oracle continues its own moments; the iterate restarts from the initialisation, as a second DESC_PGD call does
        ref2 = oracle.pgd_run(st, S0, 10, adam_m=am, adam_v=av, **cont)
        assert out["iters_run"] == ref2["iters_run"] and out["t_end"] == 50
        assert np.abs(out["S_vec"] - ref2["S_vec"]).max() <= 1e-9 and np.abs(out["w"] - ref2["w"]).max() <= 1e-9
        assert np.abs(out["adam_m"] - am).max() <= 1e-9 and np.abs(out["adam_v"] - av).max() <= 1e-9


def test_adam_state_after_per_problem_early_stop(lib, oracle):
    """The stop of iteration t is known after sweep t + 1 has run: its Adam update must not leak.  m_t, v_t and t_end reflect exactly
    iters_run updates, for a problem that stops while its neighbour runs on."""
    kw = dict(step_kind=2, lr=0.05, patience=3, stop_tol=1e-2)
    probs = [uniform(40, 0.5, 10, q=0.1, sigma=0.0), uniform(90, 0.5, 8, q=0.3)]
    refs, states = [], []
    for q in probs:
        st = oracle.build_structure(q["n"], q["ii"], q["jj"], seed=SEED)
        S0 = oracle.cycle_d(q["ii"], q["jj"], q["rij"].reshape(-1, 9), st)
        am, av = np.zeros(st["m_cycle"]), np.zeros(st["m_cycle"])
        refs.append((st, S0, oracle.pgd_run(st, S0, 300, adam_m=am, adam_v=av, **kw))); states.append((am, av))
    assert refs[0][2]["iters_run"] < 300
    mc = sum(st["m_cycle"] for st, _, _ in refs)
    for chk in (0, 3):
        adam = (np.zeros(mc), np.zeros(mc))
        _, s0, outs = run_batch(lib, probs, c_params(300, seed=SEED, check_every=chk, **kw), adam=adam)
        for (st, S0, ref), out, got_s0, (am, av) in zip(refs, outs, s0, states):
            check(out, ref, got_s0, S0, tol=1e-9)
            assert out["t_end"] == ref["iters_run"]
            assert np.abs(out["adam_m"] - am).max() <= 1e-9 and np.abs(out["adam_v"] - av).max() <= 1e-9


def test_python_wrapper(lib):
    """DESC_PGD_batch on [(Ind, RijMat), model object], Ind as float64 Fortran-ordered and as int32: the bits of the C-ABI path,
    the info keys, intact guard words."""
    from desc_amd import ConstantStepSize, DESC_PGD_batch, HybridGradient
    assert lib.GUARD
    a, b = uniform(40, 0.5, 10), uniform(90, 0.5, 8)
    _, _, outs = run_batch(lib, [a, b], c_params(20, lr=0.01, seed=SEED))
    par = lambda: dict(iters=20, Gradient=ConstantStepSize(0.01), seed=SEED, verbose=False)
    for Ind in (np.asfortranarray(a["mo"].Ind.astype(np.float64)), a["mo"].Ind.astype(np.int32)):
        S = DESC_PGD_batch([(Ind, a["mo"].RijMat), b["mo"]], par())
        assert isinstance(S, list) and len(S) == 2
        assert np.array_equal(S[0], outs[0]["S_vec"]) and np.array_equal(S[1], outs[1]["S_vec"])
        info = DESC_PGD_batch([(Ind, a["mo"].RijMat), b["mo"]], par(), return_info=True)
        for d, o in zip(info, outs):
            assert {"iters_run", "obj_vals", "average_change", "n_sample", "w"} <= set(d)
            assert np.array_equal(d["S_vec"], o["S_vec"]) and np.array_equal(d["w"], o["w"]) and np.array_equal(d["obj_vals"], o["obj"])
            assert np.array_equal(d["average_change"], o["avg"]) and d["iters_run"] == 20 and d["n_sample"] == o["n_sample"]
    # rows in another order: S_vec comes back in the caller's order
    perm = np.random.default_rng(2).permutation(a["mo"].Ind.shape[0])
    S = DESC_PGD_batch([(a["mo"].Ind[perm], a["mo"].RijMat[:, :, perm])], par())
    assert np.array_equal(S[0], outs[0]["S_vec"][perm])
    # a HybridGradient's state comes back per problem; the shared plugin object is left alone
    H = HybridGradient(0.001, 0.9, 0.999, 10)
    info = DESC_PGD_batch([a["mo"], b["mo"]], dict(iters=5, Gradient=H, seed=SEED, verbose=False), return_info=True)
    assert H.t == 0 and H.m_t is None
    for d in info:
        assert d["t_end"] == 5 and d["m_t"].shape == d["w"].shape and np.abs(d["v_t"]).max() > 0
    lib.verify_guards()


def test_refusal_launches_nothing_and_the_next_batch_works(lib, mixed, mixed_gpu):
    """(310, 0.95, seed 7) has n_sample = 70: refused with the index and the value; a valid batch afterwards is unaffected."""
    probs, _ = mixed
    big = uniform(310, 0.95, 7)
    arrs = [lib.ProblemArrays(q["n"], q["ii"], q["jj"], q["rij"]) for q in (probs[0], probs[1], big)]
    with pytest.raises(lib.DescError) as ei:
        lib.Batch(arrs, c_params(10, seed=3))
    assert ei.value.code == lib.ERR_INVALID and "problem 2" in str(ei.value) and "n_sample = 70" in str(ei.value)
    _, _, again = run_batch(lib, probs[:2], c_params(100, lr=0.01, seed=SEED))
    for k in range(2):
        _same_bits(again[k], mixed_gpu[2][k])

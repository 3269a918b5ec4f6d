"""The cycle-inconsistency kernels and their consumers on exact data (tests/exact_data_cases.py; qualified on the CPU by
tests/test_exact_data_host.py): rotations without noise, where the cycle cosine x = (tr(R_ij R_jk R_ki) - 1) / 2 sits on and beyond +-1.
Every other GPU test keeps it strictly inside, so two of the three branches of abs_acos_ext (acosh beyond 1, hypot(pi, acosh) beyond
-1), the ends of acos, weights tied in whole groups, S exactly 0 or 1 and an objective of exactly 0 are met only here.

(a) S0 at every call site -- the PGD layouts (sweep_gather.hip: k_cycle_d; pgd_layout.hip: k_layout_node and both instances of
    k_layout_node_dev), batch.hip, cemp.hip (staged and not), cemp_batch.hip, models_batch.hip -- against s0_enclosure: exactly 0, or
    within 2^-52 of 1, on the four-group data; inside the interval that any correctly rounded evaluation in any summation order falls
    into on the clean and half-turn data.
(b) The PGD sweeps on tied weights against the C oracle at the tolerances of tests/test_gpu_parity.py (check), equal iteration counts;
    the batched solver bit for bit itself from either builder, in another batch and alone, and within the same tolerances of DESC_PGD.
(c) The CEMP rounds on exact statistics: 1e-12 on the four-group data (edges whose sampled cycles are all consistent stay exactly 0),
    the measured CEMP_TOL on the clean and half-turn data, tiles on and off and CEMP_batch the same bits.
(d) The eight end-to-end calls and their batched counterparts at exact recovery, against E2E_TOL (16 times what each call's CPU oracle
    attains), compared entrywise after alignment: no acos.

The four-group and half-turn problems are deliberately NOT fed to anything that calls R2Q (the Lie-algebraic averaging of MPLS, DESC's
refinement and IRLS): R2Q.m divides the vector part by cos(theta / 2), which is 0 for a half turn, so such edges give inf / NaN by the
reference's own arithmetic.  tests/test_gpu_laa_maps.py pins that quirk at kernel level.

Run with -s: every call site prints its worst position inside the enclosure (distance to the nearer bound over the width; 0 is a value
on a bound, such as the exact 0 of a cycle whose cosine is 1), every comparison its worst error over its allowance."""
import numpy as np
import pytest

from tests import exact_data_cases as X
from tests.helpers import assert_structure_equal, c_params
from tests.test_gpu_parity import VARIANTS, check, run_gpu

pytestmark = pytest.mark.gpu

ULP1 = 2.0 ** -52
_cache = {}


def v4_bounds(S0_ref):
    """The four-group data's enclosure: consistent cycles give 0.0 exactly, the others a value within 2^-52 of 1."""
    return np.where(S0_ref == 0, 0.0, 1.0 - ULP1), np.where(S0_ref == 0, 0.0, 1.0 + ULP1)


def report(site, v, lo, hi):
    """NaN anywhere is a failure; every value inside [lo, hi]; prints the worst position."""
    v, lo, hi = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (v, lo, hi))
    assert v.shape == lo.shape and not np.isnan(v).any(), site
    pos = X.position(v, lo, hi)
    k = int(np.argmin(pos)) if pos.size else 0
    assert pos.size == 0 or pos[k] >= 0, (site, k, v[k], lo[k], hi[k])
    zero = (v == 0) & (lo == 0)                       # the exact 0 of a cosine of exactly 1 sits on its bound: counted, not ranked
    rest = pos[~zero & (hi > lo)]
    print("%-58s %7d values, %6d exactly 0 on the bound 0, worst position of the others %.3g" % (site, v.size, zero.sum(), rest.min() if rest.size else 0.5))


def ratio(what, err, allowed):
    print("%-58s %.3g of %.3g allowed (%.2g)" % (what, err, allowed, err / allowed if allowed else 0.0))
    assert err <= allowed, (what, err, allowed)


def pgd_params(iters, **kw):
    p = c_params(iters, seed=X.SEED, **kw)
    p.n_sample_min = X.NMIN
    return p


def pgd_s0_reference(oracle, name):
    """(model, marshalled arrays, oracle structure, lo, hi) of one S0 case, computed once."""
    if name not in _cache:
        kind, key = X.S0_CASES[name]
        mo = X.problem(kind, key)
        nn, ii, jj, rij = X.marshalled(mo)
        st = oracle.build_structure(nn, ii, jj, seed=X.SEED, n_sample_min=X.NMIN)
        if kind == "v4":
            lo, hi = v4_bounds(oracle.cycle_d(ii, jj, rij.reshape(-1, 9), st))
        else:
            lo, hi = X.s0_enclosure(*X.pgd_cycles(mo, st)[:3])
        _cache[name] = (mo, (nn, ii, jj, rij), st, lo, hi)
    return _cache[name]


# ---- (a) S0 at every call site -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", list(X.S0_CASES))
def test_s0_of_the_pgd_layouts(lib, oracle, name, where, monkeypatch):
    """Solver.s0() for the gather, node and band layouts; on a device-built structure also with the staged layout kernel off
    (k_layout_node_dev<., false>) and with the early layout off (the export to k_layout_node)."""
    mo, (nn, ii, jj, rij), st, lo, hi = pgd_s0_reference(oracle, name)
    prob = lib.ProblemArrays(nn, ii, jj, rij)
    combos = [(v, None, None) for v in VARIANTS] if where == "host" else [(v, s, e) for v in VARIANTS for s in "10" for e in "10"]
    for variant, staged, early in combos:
        with monkeypatch.context() as mp:
            mp.setenv("DESC_DEBUG_VARIANT", VARIANTS[variant])
            if staged is not None:
                mp.setenv("DESC_DEBUG_STAGED_LAYOUT", staged)
                mp.setenv("DESC_DEBUG_EARLY_LAYOUT", early)
            dst = lib.Structure.build(prob, X.NMIN, X.SEED, lib.BUILD_DEVICE if where == "device" else lib.BUILD_HOST, 0)
            solver = lib.Solver(prob, dst, 0)
            try:
                s0, kernel = solver.s0(), solver.kernel_name()
            finally:
                solver.destroy()
            if (variant, staged, early) == combos[0]:
                assert_structure_equal(dst.arrays(), st)
            dst.free()
        tag = "" if staged is None else " staged %s early %s" % (staged, early)
        report("%s %s %s%s [%s]" % (name, where, variant, tag, kernel.split("(")[0][:24]), s0, lo, hi)


@pytest.mark.parametrize("where", ["host", "device"])
def test_s0_of_the_batched_solver(lib, oracle, where):
    """desc_pgd_batch_get_s0 for the six cases in one batch (batch.hip), both structure builders."""
    names = list(X.S0_CASES)
    refs = [pgd_s0_reference(oracle, k) for k in names]
    arrs = [lib.ProblemArrays(*r[1]) for r in refs]
    b = lib.Batch(arrs, pgd_params(1), None, lib.BUILD_DEVICE if where == "device" else lib.BUILD_HOST)
    try:
        assert b.built_where == (lib.BUILD_DEVICE if where == "device" else lib.BUILD_HOST)
        s0 = [v.copy() for v in b.s0()]
        sts = [b.structure(k) for k in range(b.count)]
    finally:
        b.destroy()
    for k, (name, r) in enumerate(zip(names, refs)):
        assert_structure_equal(sts[k], r[2])
        report("batch %s %s" % (where, name), s0[k], r[3], r[4])


def cemp_bounds(name, ns):
    kind, key = X.CEMP_CASES[name]
    parts = X.cemp_parts(kind, key, ns, X.SEED)
    lo, hi = v4_bounds(parts.S0) if kind == "v4" else (parts.lo, parts.hi)
    return parts, np.where(parts.pos, lo, 0.0), np.where(parts.pos, hi, 0.0)


def cemp_params(ns, max_iter=6):
    return dict(max_iter=max_iter, reweighting=X.BETA, nsample=ns, seed=X.SEED)


@pytest.mark.parametrize("env", [{}, {"DESC_DEBUG_STAGED_LAYOUT": "0"}, {"DESC_DEBUG_CEMP_TILES": "0"}], ids=["default", "unstaged", "plain"])
@pytest.mark.parametrize("name", list(X.CEMP_CASES))
def test_s0_of_cemp(name, env, monkeypatch):
    """CEMP with max_iter = 0 returns the column means of S0Mat (CEMP.m:102-103): with nsample = 1 the single sample itself, otherwise
    held against the mean of the bounds; the sampled third nodes are the oracle's (the enclosure is computed from them)."""
    from desc_amd import CEMP
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mo = X.problem(*X.CEMP_CASES[name])
    for ns in X.CEMP_NSAMPLES:
        parts, lo, hi = cemp_bounds(name, ns)
        S = CEMP(mo.Ind, mo.RijMat, cemp_params(ns, 0))
        assert (S[~parts.pos] == 1.0).all()                                            # edges without a 3-cycle keep 1 (CEMP.m:103)
        mlo, mhi = (lo[0], hi[0]) if ns == 1 else X.mean_enclosure(lo, hi, axis=0)
        report("CEMP %s %s nsample %d" % (name, "/".join(env) or "default", ns), S[parts.pos], mlo[parts.pos], mhi[parts.pos])


def test_s0_of_cemp_batch(lib):
    """desc_cemp_batch_get_samples: every sampled cycle's S0 of the three cases in one batch, the sampled edges {j,k} and {k,i} the
    oracle's; CEMP_batch with max_iter = 0 the bits of CEMP."""
    from desc_amd import CEMP, CEMP_batch
    names = list(X.CEMP_CASES)
    mos = [X.problem(*X.CEMP_CASES[k]) for k in names]
    arrs = [lib.ProblemArrays(*X.marshalled(mo)) for mo in mos]
    for ns in X.CEMP_NSAMPLES:
        h = lib.CempBatch(arrs, ns, seed=X.SEED)
        try:
            smp = h.samples()
        finally:
            h.destroy()
        means = CEMP_batch(mos, cemp_params(ns, 0))
        for name, mo, s, mean in zip(names, mos, smp, means):
            parts, lo, hi = cemp_bounds(name, ns)
            assert np.array_equal(s["has_cycle"], parts.pos)
            assert np.array_equal(s["e_jk"][parts.pos], parts.Ejk.T[parts.pos]) and np.array_equal(s["e_ki"][parts.pos], parts.Eki.T[parts.pos])
            report("CEMP_batch %s nsample %d" % (name, ns), s["s0"][parts.pos], lo.T[parts.pos], hi.T[parts.pos])
            assert np.array_equal(mean, CEMP(mo.Ind, mo.RijMat, cemp_params(ns, 0))), (name, ns)


def test_s0_of_the_model_generator(lib):
    """ErrVec of Uniform_Topology_batch at q = 0, sigma = 0 (models_batch.hip): |acos((tr(Rij_orig' Rij) - 1) / 2)| / pi of two equal
    rotations, held against the enclosure computed from the blocks the call returns."""
    from desc_amd import Uniform_Topology_batch
    for mo in Uniform_Topology_batch([40, 120], [0.5, 0.6], 0.0, 0.0, seeds=[41, 42]):
        Rg = np.ascontiguousarray(np.transpose(mo.Rij_orig, (2, 1, 0)))                # Rij_orig'
        Rm = np.ascontiguousarray(np.transpose(mo.RijMat, (2, 0, 1)))
        I = np.broadcast_to(np.eye(3), Rm.shape)
        x = X.cosines_f64(Rg, Rm, I)
        print("generator n %d: %d edges, cosine above 1: %.1f %%, below: %.1f %%, exactly 1: %.1f %%"
              % (mo.n, x.size, 100 * (x > 1).mean(), 100 * (x < 1).mean(), 100 * (x == 1).mean()))
        assert not mo.corrupted.any() and (np.abs(x - 1) < 1e-14).all()
        lo, hi = X.s0_enclosure(Rg, Rm, I)
        report("Uniform_Topology_batch n %d ErrVec" % mo.n, mo.ErrVec, lo, hi)


# ---- (b) PGD on ties ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", list(X.PGD_RULES))
@pytest.mark.parametrize("pname", list(X.PGD_PROBLEMS))
def test_pgd_on_tied_weights(lib, oracle, pname, rule):
    """The three layouts against the C oracle through tests/test_gpu_parity.py's check, at its tolerances (S0 is exact on both sides);
    check asserts the iteration count.  With q = 0 the objective is exactly 0 and the patience rule fires on differences of exactly 0."""
    kw = X.PGD_RULES[rule]
    for iters in X.PGD_ITERS:
        (nn, ii, jj, rij), st, S0, ref, _ = X.pgd_reference(pname, rule, iters)
        for variant in VARIANTS:
            host_st = lib.Structure.build(lib.ProblemArrays(nn, ii, jj), X.NMIN, X.SEED, lib.BUILD_HOST, 0)          # run_gpu frees it
            arrays, s0, out = run_gpu(lib, nn, ii, jj, rij, pgd_params(iters, **kw), variant=variant, structure=host_st)
            assert_structure_equal(arrays, st)
            err = max(float(np.abs(out["S_vec"] - ref["S_vec"]).max()), float(np.abs(out["w"] - ref["w"]).max()))
            print("%-58s %.3g of %.3g allowed; iterations %d / %d; exact zeros in w %d / %d"
                  % ("PGD %s %s %s %d [%s]" % (pname, rule, variant, iters, out["kernel"].split("(")[0][:20]), err, X.PGD_TOL[rule],
                     out["iters_run"], ref["iters_run"], (out["w"] == 0).sum(), (ref["w"] == 0).sum()))
            assert np.array_equal(s0, S0)                                               # 0 and 1: nothing to round
            check(out, ref, s0, S0, tol=X.PGD_TOL[rule])
            if pname == "q0":
                assert not out["obj"].any() and not out["S_vec"].any() and out["iters_run"] == min(iters, X.PATIENCE + 1)


def _gradient(rule):
    from desc_amd import ConstantStepSize, HybridGradient
    kw = X.PGD_RULES[rule]
    return ConstantStepSize(kw["lr"]) if kw["step_kind"] == 0 else HybridGradient(kw["lr"], kw["beta1"], kw["beta2"], kw["decay_interval"])


def _run_batch(lib, probs, p, where):
    b = lib.Batch([lib.ProblemArrays(*q) for q in probs], p, None, where)
    try:
        outs, _ = b.run(p, want_w=True)
        return [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in o.items()} for o in outs]
    finally:
        b.destroy()


@pytest.mark.parametrize("rule", list(X.PGD_RULES))
def test_pgd_batch_on_tied_weights(lib, oracle, rule):
    """The three problems in one batch (desc_pgd_batch_*, n_sample_min = NMIN): the oracle's tolerances and iteration counts per
    problem and -- the contract of include/desc_amd.h and tests/test_gpu_batch.py -- the same bits from either structure builder, in the
    reversed batch and for each problem as a batch of one.  DESC_PGD_batch itself (n_sample_min 30) on the two n = 40 problems: the
    oracle's tolerances, and DESC_PGD's iteration count and S_vec at the same tolerance.

    Bit equality with DESC_PGD is not asserted: the single-problem sweeps (k_sweep_small, k_sweep_node, k_sweep_band, k_sweep) and
    batch.hip cut a segment into lanes differently and so add its terms in another order; among themselves the single-problem sweeps
    are held to 1e-12 (tests/test_gpu_parity.py).  Measured here: max |S_vec(DESC_PGD_batch) - S_vec(DESC_PGD)| = 2.2e-16 on the n = 40,
    q = 0.2 problem after one iteration at lr = 0.01."""
    from desc_amd import DESC_PGD, DESC_PGD_batch
    kw = X.PGD_RULES[rule]
    names = list(X.PGD_PROBLEMS)
    for iters in X.PGD_ITERS:
        refs = [X.pgd_reference(k, rule, iters) for k in names]
        probs = [r[0] for r in refs]
        p = pgd_params(iters, **kw)
        host = _run_batch(lib, probs, p, lib.BUILD_HOST)
        for pname, (_, st, S0, ref, _), out in zip(names, refs, host):
            err = max(float(np.abs(out["S_vec"] - ref["S_vec"]).max()), float(np.abs(out["w"] - ref["w"]).max()))
            ratio("batch %s %s %d iterations (stopped at %d, oracle %d)" % (pname, rule, iters, out["iters_run"], ref["iters_run"]), err, X.PGD_TOL[rule])
            assert out["iters_run"] == ref["iters_run"] and out["n_sample"] == st["n_sample"]
            assert np.allclose(out["obj"], ref["obj"], rtol=1e-12, atol=1e-9) and np.allclose(out["avg"], ref["avg"], rtol=1e-9, atol=1e-14)
        others = [_run_batch(lib, probs, p, lib.BUILD_DEVICE), _run_batch(lib, probs[::-1], p, lib.BUILD_HOST)[::-1]]
        others.append([_run_batch(lib, [q], p, lib.BUILD_HOST)[0] for q in probs])
        for other in others:
            for a, b in zip(host, other):
                assert a["iters_run"] == b["iters_run"] and all(np.array_equal(a[k], b[k]) for k in ("S_vec", "w", "obj", "avg"))
        par = lambda: dict(iters=iters, Gradient=_gradient(rule), seed=X.SEED, verbose=False, build_where=lib.BUILD_HOST)      # noqa: E731
        small = [k for k in names if X.PGD_PROBLEMS[k][1][0] == 40]
        mos = [X.problem(*X.PGD_PROBLEMS[k]) for k in small]
        for pname, mo, d in zip(small, mos, DESC_PGD_batch(mos, par(), return_info=True)):
            ref = X.pgd_reference(pname, rule, iters)[3]
            S1, info1 = DESC_PGD(mo.Ind, mo.RijMat, par(), return_info=True)
            assert d["iters_run"] == ref["iters_run"] == info1["iters_run"]
            ratio("DESC_PGD_batch %s %s %d against the oracle" % (pname, rule, iters), float(np.abs(d["S_vec"] - ref["S_vec"]).max()), X.PGD_TOL[rule])
            ratio("DESC_PGD_batch %s %s %d against DESC_PGD" % (pname, rule, iters), float(np.abs(d["S_vec"] - S1).max()), X.PGD_TOL[rule])


# ---- (c) CEMP rounds on exact statistics ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.CEMP_CASES))
def test_cemp_rounds_on_exact_statistics(name, monkeypatch):
    """Six rounds at the three nsample classes of cemp_edge_round: weights exp(0) = 1 across whole edges, S exactly 0 or 1 on many.
    Four-group data at the suite's 1e-12, clean and half-turn data at the measured CEMP_TOL; tiles on and off and CEMP_batch the same
    bits; an edge all of whose sampled cycles are consistent stays exactly 0 (the four-group data); corrupted edges stay apart from
    clean ones wherever the oracle keeps them apart."""
    from desc_amd import CEMP, CEMP_batch
    kind, key = X.CEMP_CASES[name]
    mo = X.problem(kind, key)
    tol = 1e-12 if kind == "v4" else X.CEMP_TOL[name]
    for ns in X.CEMP_NSAMPLES:
        parts = X.cemp_parts(kind, key, ns, X.SEED)
        ref = X.cemp_variants(kind, key, ns, X.SEED)[0]
        S = CEMP(mo.Ind, mo.RijMat, cemp_params(ns))
        assert np.isfinite(S).all() and (S[~parts.pos] == 1.0).all()
        ratio("CEMP %s nsample %d, six rounds" % (name, ns), float(np.abs(S - ref).max()), tol)
        with monkeypatch.context() as mp:
            mp.setenv("DESC_DEBUG_CEMP_TILES", "0")
            assert np.array_equal(CEMP(mo.Ind, mo.RijMat, cemp_params(ns)), S), ns
        assert np.array_equal(CEMP_batch([mo], cemp_params(ns))[0], S), ns
        if kind == "v4":
            allzero = parts.pos & (parts.S0 == 0).all(axis=0)
            assert allzero.sum() >= 5 and (ref[allzero] == 0.0).all() and (S[allzero] == 0.0).all()
        good, bad = parts.pos & ~mo.corrupted, parts.pos & mo.corrupted
        if ref[good].max() < ref[bad].min():
            print("    clean edges at most %.3g (oracle %.3g), corrupted at least %.3g (oracle %.3g)" % (S[good].max(), ref[good].max(), S[bad].min(), ref[bad].min()))
            assert S[good].max() < S[bad].min()
            gap = 0.5 * (ref[good].max() + ref[bad].min())
            assert np.array_equal(S > gap, ref > gap)


# ---- (d) end to end at exact recovery ------------------------------------------------------------------------------------------------
DEFECT = dict(Spectral=1e-12, CEMP_GCW=1e-12, CEMP_MST=1e-12, DESC_init=1e-12,      # tests/test_gpu_spectral.py, tests/test_gpu_cemp_batch.py: assert_rotations
              MPLS=1e-6, DESC=1e-6, IRLS_GM=1e-6, IRLS_L12=1e-6)                    # tests/test_gpu_mpls.py, tests/test_gpu_irls.py: q2R of an unnormalised quaternion


def _desc_params(lib):
    from desc_amd import ConstantStepSize
    return dict(iters=X.E2E_PGD["iters"], Gradient=ConstantStepSize(X.E2E_PGD["lr"]), learning_rate=X.E2E_PGD["lr"], seed=X.SEED, verbose=False,
                make_plots=False, build_where=lib.BUILD_HOST)


def single_call(lib, call, mo):
    """(R, what the oracle's counts are compared with, everything the batch is compared with) of one call on one problem."""
    import desc_amd as D
    cemp, mpls = X.demo_params()
    if call == "Spectral":
        R, info = D.Spectral(mo.Ind, mo.RijMat, return_info=True)
        assert info["converged"]
        return R, {}, {}
    if call == "CEMP_GCW":
        R, info = D.CEMP_GCW(mo.Ind, mo.RijMat, cemp, return_info=True)
        assert info["converged"]
        return R, {}, dict(S=D.CEMP(mo.Ind, mo.RijMat, cemp))
    if call == "CEMP_MST":
        S = D.CEMP(mo.Ind, mo.RijMat, cemp)
        return D.MST(mo.Ind, mo.RijMat, S), {}, dict(S=S)
    if call == "MPLS":
        R, R_init, info = D.MPLS(mo.Ind, mo.RijMat, cemp, mpls, return_info=True)
        assert info["cg_unconverged"] == 0
        return R, dict(iters=info["iters"]), dict(R_init=R_init, S=info["SVec"], iters=info["iters"])
    if call == "DESC_init":
        R, S, info = D.DESC_init(mo.Ind, mo.RijMat, _desc_params(lib), return_info=True)
        assert info["gcw"]["converged"]
        return R, dict(pgd_iters=info["pgd"]["iters_run"]), dict(S=S)
    if call == "DESC":
        R, R_init, S, info = D.DESC(mo.Ind, mo.RijMat, _desc_params(lib), return_info=True)
        assert info["gcw"]["converged"] and info["refine"]["cg_unconverged"] == 0
        return R, dict(iters=info["refine"]["iters"], pgd_iters=info["pgd"]["iters_run"]), dict(S=S, R_init=R_init, iters=info["refine"]["iters"])
    R, info = dict(IRLS_GM=D.IRLS_GM, IRLS_L12=D.IRLS_L12)[call](mo.RijMat, mo.Ind, return_info=True)
    assert info["cg_unconverged"] == 0
    return R, dict(l1_iters=info["l1_iters"], irls_iters=info["irls_iters"]), dict(R_l1=info["R_l1"], l1_iters=info["l1_iters"], irls_iters=info["irls_iters"])


def batch_call(lib, call, mos):
    """The batched counterpart on the two problems in one batch: per problem (R, everything compared with the single call)."""
    import desc_amd as D
    cemp, mpls = X.demo_params()
    seeds = [X.SEED] * len(mos)
    if call == "Spectral":
        return [(R, {}) for R, info in D.Spectral_batch(mos, return_info=True)]
    if call == "CEMP_GCW":
        return [(R, dict(S=S)) for R, S, info in D.CEMP_GCW_batch(mos, cemp, seeds=seeds, return_info=True)]
    if call == "CEMP_MST":
        return [(R, dict(S=S)) for R, S, info in D.CEMP_MST_batch(mos, cemp, seeds=seeds, return_info=True)]
    if call == "MPLS":
        return [(R, dict(R_init=R_init, S=info["SVec"], iters=info["mpls"]["iters"])) for R, R_init, info in D.MPLS_batch(mos, cemp, mpls, seeds=seeds, return_info=True)]
    if call == "DESC_init":
        return [(R, dict(S=S)) for R, S, info in D.DESC_init_batch(mos, _desc_params(lib), seeds=seeds, return_info=True)]
    if call == "DESC":
        return [(R, dict(S=S, R_init=R_init, iters=info["refine"]["iters"]))
                for R, R_init, S, info in D.DESC_batch(mos, _desc_params(lib), seeds=seeds, return_info=True)]
    fn = dict(IRLS_GM=D.IRLS_GM_batch, IRLS_L12=D.IRLS_L12_batch)[call]
    return [(R, dict(R_l1=info["R_l1"], l1_iters=info["l1_iters"], irls_iters=info["irls_iters"])) for R, info in fn(mos, return_info=True)]


# How a batch entry is held against the single call, by the contract its own test module states: the eigen-solves agree after alignment
# at 1e-8 (tests/test_gpu_gcw_batch.py, tests/test_gpu_cemp_batch.py), and what follows an eigen-solve inherits its gauge (the
# refinement at the 1e-7 of tests/test_gpu_refine_batch.py's oracle comparison); everything else is bit for bit (tests/test_gpu_batch.py,
# tests/test_gpu_cemp_batch.py, tests/test_gpu_mpls_batch.py, tests/test_gpu_irls_batch.py).  S_vec of DESC_init_batch / DESC_batch is
# DESC_PGD_batch's, which agrees with DESC_PGD's within the sweep tolerance 1e-10, not in every bit (test_pgd_batch_on_tied_weights).
ALIGNED = dict(Spectral=dict(R=1e-8), CEMP_GCW=dict(R=1e-8), DESC_init=dict(R=1e-8), DESC=dict(R=1e-7, R_init=1e-8))
CLOSE = dict(DESC_init=dict(S=1e-10), DESC=dict(S=1e-10))


@pytest.mark.parametrize("call", X.E2E_CALLS)
def test_end_to_end_at_exact_recovery(lib, oracle, call):
    from oracle.spectral_oracle import rotation_alignment
    cases = list(X.E2E_CASES)
    mos = [X.problem(*X.E2E_CASES[c]) for c in cases]
    singles = []
    for case, mo in zip(cases, mos):
        ref = X.e2e_oracle(call, case)
        R, counts, rest = single_call(lib, call, mo)
        singles.append((R, rest))
        assert np.isfinite(R).all() and R.shape == (3, 3, mo.n)
        ratio("%s %s SO(3) defect" % (call, case), X.so3_defect(R), DEFECT[call])
        ratio("%s %s aligned max|R - R_orig| (oracle attains %.3g)" % (call, case, X.aligned_error(ref["R"], mo.R_orig)),
              X.aligned_error(R, mo.R_orig), X.E2E_TOL[case][call])
        if call == "Spectral":                                                       # its E2E_TOL says nothing at q = 0.2: the dense oracle does
            ratio("Spectral %s aligned max|R - oracle|" % case, float(np.abs(rotation_alignment(R, ref["R"])[0] - ref["R"]).max()), 1e-8)
        for k, v in counts.items():
            print("    %s %s %s: %d (oracle %d)" % (call, case, k, v, ref[k]))
            assert v == ref[k], (call, case, k, v, ref[k])
        if call == "DESC":
            assert counts["iters"] == 1
    for case, mo, (R, rest), (R1, rest1) in zip(cases, mos, batch_call(lib, call, mos), singles):
        assert np.isfinite(R).all()
        ratio("%s_batch %s SO(3) defect" % (call, case), X.so3_defect(R), DEFECT[call])
        ratio("%s_batch %s aligned max|R - R_orig|" % (call, case), X.aligned_error(R, mo.R_orig), X.E2E_TOL[case][call])
        both = dict(rest, R=R), dict(rest1, R=R1)
        for k in both[0]:
            a, b = both[0][k], both[1][k]
            if k in ALIGNED.get(call, {}):
                ratio("%s_batch %s %s against the single call, aligned" % (call, case, k), float(np.abs(rotation_alignment(a, b)[0] - b).max()), ALIGNED[call][k])
            elif k in CLOSE.get(call, {}):
                ratio("%s_batch %s %s against the single call" % (call, case, k), float(np.abs(a - b).max()), CLOSE[call][k])
            else:
                assert np.array_equal(a, b), (call, case, k)

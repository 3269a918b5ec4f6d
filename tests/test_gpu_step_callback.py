"""User-defined params.Gradient plugins on the GPU: the two-phase iteration (gradient pass | GetStep | apply pass, the cut at
DESC_PGD.m:207) against the CPU oracle, the literal restatement and the library's own native rules, on every layout.

Tolerances are those of tests/test_gpu_parity.py::check: S_vec and w 1e-10 (1e-9 for Adam, whose 1/(sqrt(v)+1e-8) amplifies
round-off), obj rtol 1e-12 / atol 1e-9, avg rtol 1e-9 / atol 1e-14, iters_run equal."""
import os

import numpy as np
import pytest

from tests.helpers import c_params, make_problem, oracle_reference

pytestmark = pytest.mark.gpu
TOL = 1e-10
VARIANTS = {"band": "3", "node": "2", "gather": "1"}     # DESC_DEBUG_VARIANT, as tests/test_gpu_parity.py
ALL_VARIANTS = ["band", "node", "gather"]


def make_solver(lib, nn, ii, jj, rij, seed, variant, nmin=30, rank=0, world=1):
    os.environ["DESC_DEBUG_VARIANT"] = VARIANTS[variant]
    try:
        prob = lib.ProblemArrays(nn, ii, jj, rij)
        st = lib.Structure.build(prob, nmin, seed, lib.BUILD_HOST, 0)
        try:
            return lib.Solver(prob, st, 0, rank, world)
        finally:
            st.free()
    finally:
        os.environ.pop("DESC_DEBUG_VARIANT", None)


def run_external(lib, nn, ii, jj, rij, p, G, variant, nmin=30):
    solver = make_solver(lib, nn, ii, jj, rij, p.seed, variant, nmin)
    try:
        s0 = solver.s0()
        out = solver.run_external(p, G.GetStep, device_tensors=bool(getattr(G, "device_tensors", False)), want_w=True)
    finally:
        solver.destroy()
    return s0, out


def run_native(lib, nn, ii, jj, rij, p, variant, adam=None, nmin=30):
    solver = make_solver(lib, nn, ii, jj, rij, p.seed, variant, nmin)
    try:
        return solver.run(p, want_w=True, adam=adam)
    finally:
        solver.destroy()


def check(out, ref, tol=TOL, what=""):
    d = dict(S=np.abs(out["S_vec"] - ref["S_vec"]).max(), w=np.abs(out["w"] - ref["w"]).max(),
             obj=np.abs(np.asarray(out["obj"]) - np.asarray(ref["obj"])[:len(out["obj"])]).max() if len(out["obj"]) == len(ref["obj"]) else np.nan)
    print(f"{what}: iters {out['iters_run']} / {ref['iters_run']}  max|dS| {d['S']:.3e}  max|dw| {d['w']:.3e}  max|dobj| {d['obj']:.3e}")
    assert out["iters_run"] == ref["iters_run"]
    assert d["S"] <= tol
    assert d["w"] <= tol
    assert np.allclose(out["obj"], ref["obj"], rtol=1e-12, atol=1e-9)
    assert np.allclose(out["avg"], ref["avg"], rtol=1e-9, atol=1e-14)


# ---------------------------------------------------------------- plugins --
class W:
    """A thin wrapper around a rule the library knows: no subclass of it, so it takes the external path."""

    def __init__(self, g):
        self.g, self.calls = g, 0

    def GetStep(self, grad):
        self.calls += 1
        return self.g.GetStep(grad)


class Plain:
    def __init__(self, lr):
        self.lr, self.calls = lr, 0

    def GetStep(self, grad):
        self.calls += 1
        return -self.lr * grad


class Momentum:
    """(a) heavy ball: v = 0.9 v - lr g."""

    def __init__(self, lr=0.01, mu=0.9):
        self.lr, self.mu, self.v = lr, mu, None

    def GetStep(self, grad):
        self.v = -self.lr * grad if self.v is None else self.mu * self.v - self.lr * grad
        return self.v


class Positional:
    """(b) depends on the cycle's position in the reference's order: catches a leaked layout order."""

    def __init__(self, lr=0.01):
        self.lr, self.f = lr, None

    def GetStep(self, grad):
        if self.f is None:
            self.f = 1 + 0.5 * np.sin(np.arange(grad.shape[0]))
        return -self.lr * grad * self.f


class Clipped:
    """(c) global-norm clipping: step = -lr grad / max(1, |grad|_2 / c)."""

    def __init__(self, lr, c):
        self.lr, self.c, self.norms = lr, c, []

    def GetStep(self, grad):
        nrm = float(np.sqrt(np.sum(grad * grad)))
        self.norms.append(nrm)
        return -self.lr * grad / max(1.0, nrm / self.c)


class TorchChecks:
    device_tensors = True
    m_cycle = None

    def look(self, grad):
        import torch
        assert grad.is_cuda and grad.dtype == torch.float64 and grad.dim() == 1
        assert self.m_cycle is None or grad.numel() == self.m_cycle
        return torch


class TorchPlain(TorchChecks):
    def __init__(self, lr, m_cycle=None):
        self.lr, self.m_cycle = lr, m_cycle

    def GetStep(self, grad):
        self.look(grad)
        return -self.lr * grad


class TorchMomentum(TorchChecks):
    def __init__(self, lr=0.01, mu=0.9, m_cycle=None):
        self.lr, self.mu, self.v, self.m_cycle = lr, mu, None, m_cycle

    def GetStep(self, grad):
        self.look(grad)
        self.v = -self.lr * grad if self.v is None else self.mu * self.v - self.lr * grad
        return self.v


class TorchPositional(TorchChecks):
    def __init__(self, lr=0.01, m_cycle=None):
        self.lr, self.f, self.m_cycle = lr, None, m_cycle

    def GetStep(self, grad):
        torch = self.look(grad)
        if self.f is None:          # the factor of the NumPy rule, bit for bit (a device sin may round differently)
            self.f = torch.from_numpy(1 + 0.5 * np.sin(np.arange(grad.numel()))).to(grad.device)
        return -self.lr * grad * self.f


# problem of tests/test_gpu_parity.py::test_step_plugins
def plugins_problem():
    return make_problem("uniform", n=90, p=0.5, q=0.3, sigma=0.1, seed=8)


KNOWN = {
    "constant": (lambda S: S.ConstantStepSize(1.0), dict(step_kind=0, lr=1.0)),
    "piecewise": (lambda S: _with_t(S.PiecewiseStepSize(0.05, 7), 3), dict(step_kind=1, lr=0.05, decay_interval=7, t0=3)),
    "hybrid_adam": (lambda S: S.HybridGradient(0.001, .9, .999, 10), dict(step_kind=2, lr=0.001, beta1=0.9, beta2=0.999, decay_interval=10)),
    "hybrid_plain": (lambda S: _with_t(S.HybridGradient(0.001, .9, .999, 10).stopAdam(), 4),
                     dict(step_kind=2, lr=0.001, beta1=0.9, beta2=0.999, decay_interval=10, hybrid_strategy=1, t0=4)),
}


def _with_t(g, t):
    g.t = t
    return g


@pytest.mark.parametrize("variant", ALL_VARIANTS)
@pytest.mark.parametrize("kind", list(KNOWN))
def test_known_rules_through_the_callback_path(lib, oracle, kind, variant):
    """The three rules of Utils/ wrapped so that the library does not recognise them: oracle, native path and callback path agree."""
    from desc_amd import stepsize
    mo, nn, ii, jj, rij = plugins_problem()
    make, kw = KNOWN[kind]
    iters = 40
    st, S0, ref = oracle_reference(oracle, nn, ii, jj, rij, seed=5, iters=iters, **kw)
    G = W(make(stepsize))
    t0 = getattr(G.g, "t", 0)
    s0, out = run_external(lib, nn, ii, jj, rij, c_params(iters, seed=5), G, variant)
    assert np.abs(s0 - S0).max() <= 1e-14
    tol = 1e-9 if kind == "hybrid_adam" else TOL
    check(out, ref, tol, f"{kind}/{variant} external vs oracle")
    mc = st["m_cycle"]
    adam = (np.zeros(mc), np.zeros(mc)) if kind == "hybrid_adam" else None
    nat = run_native(lib, nn, ii, jj, rij, c_params(iters, seed=5, **kw), variant, adam=adam)
    check(out, nat, tol, f"{kind}/{variant} external vs native")
    assert G.calls == out["iters_run"] == out["calls"]
    if kind != "constant":
        assert G.g.t == t0 + out["iters_run"] == nat["t_end"]
    assert out["t_end"] == out["iters_run"]                      # the library keeps no counter for a rule it does not know (t0 = 0)
    if kind == "hybrid_adam":
        print(f"adam state external vs native: max|dm| {np.abs(G.g.m_t - nat['adam_m']).max():.3e}  max|dv| {np.abs(G.g.v_t - nat['adam_v']).max():.3e}")
        assert np.abs(G.g.m_t - nat["adam_m"]).max() <= tol and np.abs(G.g.v_t - nat["adam_v"]).max() <= tol


# ------------------------------------------------ rules the library has never seen --
_LITERAL = {}
CLIP_LR, CLIP_C = 0.01, 40.0


def new_rules():
    return dict(momentum=lambda: Momentum(0.01), positional=lambda: Positional(0.01), clipped=lambda: Clipped(CLIP_LR, CLIP_C), plain=lambda: Plain(0.01))


PROBLEMS = {
    "n90": (dict(n=90, p=0.5, q=0.3, sigma=0.1, seed=8), 5, 40),          # codegree ~ 22 < n_sample 30: all but a few dozen edges keep every cycle
    "n200": (dict(n=200, p=0.5, q=0.2, sigma=0.1, seed=4), 11, 15),       # the sampled regime (codegree ~ 50 >= n_sample 30)
}


def literal(oracle, pname, rule):
    """desc_pgd_literal on (problem, rule), computed once per session: it is interpreted NumPy over dense n x m_pos arrays."""
    if (pname, rule) not in _LITERAL:
        from oracle.desc_pgd_literal import desc_pgd_literal
        kw, sseed, iters = PROBLEMS[pname]
        mo, nn, ii, jj, rij = make_problem("uniform", **kw)
        G = new_rules()[rule]()
        S, state = desc_pgd_literal(mo.Ind, mo.RijMat, iters, G, sampler=oracle.keyed_sampler(sseed), return_state=True)
        _LITERAL[(pname, rule)] = (S, state, G)
    return _LITERAL[(pname, rule)]


@pytest.mark.parametrize("variant", ALL_VARIANTS)
@pytest.mark.parametrize("pname", list(PROBLEMS))
@pytest.mark.parametrize("rule", ["momentum", "positional", "clipped"])
def test_new_rules_match_the_literal_restatement(lib, oracle, rule, pname, variant):
    kw, sseed, iters = PROBLEMS[pname]
    mo, nn, ii, jj, rij = make_problem("uniform", **kw)
    S_ref, state, G_ref = literal(oracle, pname, rule)
    if pname == "n200":
        assert int(np.diff(state["cum_ind"]).max()) == state["n_sample"] and (state["CoDeg_vec"] >= state["n_sample"]).any()      # edges were sampled
    if rule == "positional":          # the rule must change the answer, else a leaked layout order would go unseen
        S_plain, _, _ = literal(oracle, pname, "plain")
        assert np.abs(S_ref - S_plain).max() > 1e-6
    if rule == "clipped":             # clipping is active in the first iterations
        assert all(nrm > CLIP_C for nrm in G_ref.norms[:3]), G_ref.norms[:3]
    G = new_rules()[rule]()
    s0, out = run_external(lib, nn, ii, jj, rij, c_params(iters, seed=sseed), G, variant)
    assert out["w"].shape[0] == state["m_cycle"] and np.abs(s0 - state["S0_long"]).max() <= 1e-14
    dS, dw = np.abs(out["S_vec"] - S_ref).max(), np.abs(out["w"] - state["wijk"]).max()
    print(f"{rule}/{pname}/{variant}: max|dS| {dS:.3e}  max|dw| {dw:.3e}  iters {out['iters_run']}")
    assert out["iters_run"] == state["iters_run"]
    assert dS <= TOL and dw <= TOL
    assert np.allclose(out["obj"], state["obj_vals"], rtol=1e-12, atol=1e-9)
    assert np.allclose(out["avg"], state["avg_changes"], rtol=1e-9, atol=1e-14)
    if rule == "clipped":
        assert np.allclose(G.norms, G_ref.norms, rtol=1e-9)


@pytest.mark.parametrize("variant", ALL_VARIANTS)
@pytest.mark.parametrize("n,p,nmin", [(150, 0.9, 100), (260, 0.92, 250), (330, 0.97, 300)])
def test_long_segments(lib, oracle, n, p, nmin, variant):
    """Segments of 65..128, 129..256 and more than 256 cycles (the last: always the gather layout, multi-pass kernels).  The plain rule
    against the oracle's constant rule; the positional rule, which the oracle does not have, against the gather layout of the same
    library, whose cycle order is the reference's own."""
    mo, nn, ii, jj, rij = make_problem("uniform", n=n, p=p, q=0.25, sigma=0.1, seed=n)
    st = oracle.build_structure(nn, ii, jj, seed=9, n_sample_min=nmin)
    S0 = oracle.cycle_d(ii, jj, rij.reshape(-1, 9), st)
    ref = oracle.pgd_run(st, S0, 12, step_kind=0, lr=0.01)
    mx = int(np.diff(st["cum_ind"]).max())
    assert mx > 64
    s0, out = run_external(lib, nn, ii, jj, rij, c_params(12, seed=9), Plain(0.01), variant, nmin=nmin)
    assert np.abs(s0 - S0).max() <= 1e-14
    check(out, ref, TOL, f"plain/{n}/{variant} (longest segment {mx}) external vs oracle")
    _, pos = run_external(lib, nn, ii, jj, rij, c_params(12, seed=9), Positional(0.01), variant, nmin=nmin)
    _, pos_g = run_external(lib, nn, ii, jj, rij, c_params(12, seed=9), Positional(0.01), "gather", nmin=nmin)
    assert np.abs(pos["S_vec"] - out["S_vec"]).max() > 1e-6
    check(pos, pos_g, TOL, f"positional/{n}/{variant} vs the gather layout")


@pytest.mark.parametrize("variant", ALL_VARIANTS)
def test_early_stop_and_call_count(lib, oracle, variant):
    """The problem of test_early_stop_matches_oracle: GetStep runs exactly iters_run times (:207 comes before the stop test of the
    same iteration), and the stopped handle refuses further steps."""
    mo, nn, ii, jj, rij = make_problem("uniform", n=40, p=0.5, q=0.1, sigma=0.0, seed=10)
    st, S0, ref = oracle_reference(oracle, nn, ii, jj, rij, seed=1, iters=400, lr=1.0, patience=5, stop_tol=1e-3)
    assert ref["iters_run"] < 400
    G = Plain(1.0)
    solver = make_solver(lib, nn, ii, jj, rij, 1, variant)
    try:
        out = solver.run_external(c_params(400, seed=1, patience=5, stop_tol=1e-3), G.GetStep, want_w=True)
        assert G.calls == ref["iters_run"] == out["iters_run"] == out["calls"] and out["iters_run"] < 400
        check(out, ref, TOL, f"early stop/{variant}")
        step = np.zeros(solver.m_cycle)
        for call in (lambda: solver.ext_apply(step), lambda: solver.ext_grad(step)):
            with pytest.raises(lib.DescError) as e:
                call()
            assert e.value.code == lib.ERR_STATE and "stop rule" in str(e.value)
        again = solver.download(want_w=True)                     # the result stays downloadable
        assert again["iters_run"] == out["iters_run"] and np.array_equal(again["S_vec"], out["S_vec"])
    finally:
        solver.destroy()


# ------------------------------------------------------------------ device mode --
@pytest.mark.parametrize("variant", ALL_VARIANTS)
def test_device_mode(lib, oracle, variant):
    import torch
    mo, nn, ii, jj, rij = plugins_problem()
    p = c_params(40, seed=5)
    mc = make_solver(lib, nn, ii, jj, rij, 5, variant)
    m_cycle = mc.m_cycle
    mc.destroy()
    for name, host_rule, dev_rule, exact in (("constant", Plain(1.0), TorchPlain(1.0, m_cycle), True),
                                             ("positional", Positional(0.01), TorchPositional(0.01, m_cycle), True),
                                             ("momentum", Momentum(0.01), TorchMomentum(0.01, 0.9, m_cycle), False)):
        _, a = run_external(lib, nn, ii, jj, rij, p, host_rule, variant)
        _, b = run_external(lib, nn, ii, jj, rij, p, dev_rule, variant)
        print(f"device mode {name}/{variant}: max|dS| {np.abs(a['S_vec'] - b['S_vec']).max():.3e}")
        assert a["iters_run"] == b["iters_run"] == 40
        if exact:          # the same IEEE multiplies on the same gradient
            for key in ("S_vec", "w", "obj", "avg"):
                assert np.array_equal(a[key], b[key]), (name, key)
        else:
            check(b, a, TOL, f"momentum device vs host/{variant}")

    class Bad(TorchChecks):
        def __init__(self, how):
            self.how = how

        def GetStep(self, grad):
            return dict(cpu=lambda: (-0.01 * grad).cpu(), f32=lambda: (-0.01 * grad).float(), short=lambda: (-0.01 * grad)[:-1],
                        numpy=lambda: (-0.01 * grad).cpu().numpy())[self.how]()

    for how in ("cpu", "f32", "short", "numpy"):
        with pytest.raises(ValueError):
            run_external(lib, nn, ii, jj, rij, p, Bad(how), variant)
    assert torch.cuda.is_available()


# ------------------------------------------------------------ failure containment --
@pytest.mark.parametrize("variant", ALL_VARIANTS)
def test_exception_in_getstep_propagates_and_leaves_the_process_usable(lib, variant, monkeypatch):
    from desc_amd import DESC_PGD, ConstantStepSize
    assert lib.GUARD                                             # guard words around every caller buffer are verified after each native call
    monkeypatch.setenv("DESC_DEBUG_VARIANT", VARIANTS[variant])
    mo, nn, ii, jj, rij = plugins_problem()
    native = lambda: DESC_PGD(mo.Ind, mo.RijMat, dict(iters=20, Gradient=ConstantStepSize(0.01), seed=5, verbose=False), return_info=True)[0]      # noqa: E731
    before = native()

    class Boom:
        calls = 0

        def GetStep(self, grad):
            self.calls += 1
            if self.calls == 3:
                raise RuntimeError("boom")
            return -0.01 * grad

    G = Boom()
    with pytest.raises(RuntimeError, match="^boom$"):
        DESC_PGD(mo.Ind, mo.RijMat, dict(iters=20, Gradient=G, seed=5, verbose=False))
    assert G.calls == 3
    with pytest.raises(ValueError, match="entries"):             # a step of the wrong length is refused before it reaches the library
        DESC_PGD(mo.Ind, mo.RijMat, dict(iters=20, Gradient=_ShortStep(), seed=5, verbose=False))
    assert np.array_equal(native(), before)
    lib.verify_guards()


class _ShortStep:
    def GetStep(self, grad):
        return -0.01 * grad[:-1]


# ---------------------------------------------------------------- public wrappers --
@pytest.mark.parametrize("variant", ALL_VARIANTS)
def test_public_wrappers(lib, variant, monkeypatch, capfd):
    from desc_amd import DESC, DESC_PGD, ConstantStepSize, DESC_init
    monkeypatch.setenv("DESC_DEBUG_VARIANT", VARIANTS[variant])
    mo, nn, ii, jj, rij = make_problem("uniform", n=70, p=0.5, q=0.2, sigma=0.1, seed=23)
    prm = lambda G, **kw: dict(iters=30, Gradient=G, seed=2, verbose=False, **kw)      # noqa: E731
    R_est, R_init, S_vec = DESC(mo.Ind, mo.RijMat, prm(Momentum()))
    assert R_est.shape == R_init.shape == (3, 3, nn) and S_vec.shape == (len(ii),) and np.isfinite(R_est).all()
    S_pgd, info = DESC_PGD(mo.Ind, mo.RijMat, prm(Momentum()), return_info=True)
    assert np.array_equal(S_vec, S_pgd)
    assert info["iters_run"] == 30 and info["calls"] == 30 and len(info["obj"]) == 30 and info["m_cycle"] > 0
    R0, S0 = DESC_init(mo.Ind, mo.RijMat, prm(Momentum()))
    assert np.array_equal(R0, R_init) and np.array_equal(S0, S_vec)
    # make_plots through the same loop: the keys of the native traced run, for the wrapped constant rule its numbers
    plots = dict(make_plots=True, ErrVec=mo.ErrVec, R_orig=mo.R_orig)
    Sx, ext = DESC_PGD(mo.Ind, mo.RijMat, prm(W(ConstantStepSize(0.01)), **plots), return_info=True)
    Sn, nat = DESC_PGD(mo.Ind, mo.RijMat, prm(ConstantStepSize(0.01), **plots), return_info=True)
    assert ext["iters_run"] == nat["iters_run"] == 30 and np.abs(Sx - Sn).max() <= TOL
    for key in ("svec_errors", "MSE_means", "MSE_medians"):
        assert len(ext[key]) == ext["iters_run"]
        print(f"make_plots {key}/{variant}: max rel diff {np.max(np.abs(ext[key] - nat[key]) / np.abs(nat[key])):.3e}")
        assert np.allclose(ext[key], nat[key], rtol=1e-9, atol=0), key
    # unsorted Ind: perm affects the edge vectors only
    perm = np.random.default_rng(1).permutation(mo.Ind.shape[0])
    S_perm = DESC_PGD(mo.Ind[perm], np.ascontiguousarray(mo.RijMat[:, :, perm]), prm(Momentum()))
    assert np.array_equal(S_perm, S_pgd[perm])
    # the reference's progress line, once per applied step
    capfd.readouterr()
    DESC_PGD(mo.Ind, mo.RijMat, dict(iters=6, Gradient=Momentum(), seed=2, verbose=True))
    lines = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith("iter ")]
    assert len(lines) == 6 and lines[0].startswith("iter 1: average change in S_vec ") and "objective value: " in lines[-1]


# --------------------------------------------------------------- ABI order errors --
@pytest.mark.parametrize("variant", ALL_VARIANTS)
def test_abi_order_errors(lib, variant):
    """Argument checks made on the host before any launch: none of these may fault."""
    mo, nn, ii, jj, rij = plugins_problem()
    solver = make_solver(lib, nn, ii, jj, rij, 5, variant)
    buf = lib.out_buffer(solver.m_cycle)

    def state_error(call, text):
        with pytest.raises(lib.DescError) as e:
            call()
        assert e.value.code == lib.ERR_STATE and text in str(e.value), str(e.value)

    try:
        state_error(lambda: solver.ext_grad(buf), "desc_pgd_ext_begin")                  # before begin
        state_error(lambda: solver.ext_apply(buf), "desc_pgd_ext_begin")
        with pytest.raises(lib.DescError) as e:
            solver.ext_begin(c_params(5, seed=5))                                        # step_kind must be DESC_STEP_EXTERNAL
        assert e.value.code == lib.ERR_INVALID
        solver.ext_begin(c_params(5, step_kind=lib.STEP_EXTERNAL, seed=5))
        state_error(lambda: solver.ext_apply(buf), "desc_pgd_ext_grad")                  # apply before grad
        state_error(lambda: solver.iterate(1), "caller-supplied")
        solver.ext_grad(buf)
        assert np.isfinite(buf).all() and np.abs(buf).max() > 0
        with pytest.raises(lib.DescError) as e:
            solver.ext_apply(buf, where=7)
        assert e.value.code == lib.ERR_INVALID
        avg, obj, stopped = solver.ext_apply(np.ascontiguousarray(-0.01 * buf[:solver.m_cycle]))
        assert avg > 0 and obj > 0 and not stopped
        state_error(lambda: solver.ext_apply(buf), "desc_pgd_ext_grad")                  # one step per gradient
        out = solver.download()
        assert out["iters_run"] == 1 and out["t_end"] == 1 and out["obj"][0] == obj and out["avg"][0] == avg
        gp, ap, op = solver.ext_laps()
        assert gp > 0 and ap > 0 and op > 0
    finally:
        solver.destroy()
    if variant == "gather":
        return                                               # sharding needs the node layout
    sharded = make_solver(lib, nn, ii, jj, rij, 5, variant, rank=0, world=2)
    try:
        state_error(lambda: sharded.ext_begin(c_params(5, step_kind=lib.STEP_EXTERNAL, seed=5)), "sharded")
        state_error(lambda: sharded.ext_grad(buf), "sharded")
        state_error(lambda: sharded.ext_apply(buf), "sharded")
    finally:
        sharded.destroy()

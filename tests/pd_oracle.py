"""ORACLE -- test infrastructure only.  Two references for the L1 stage's primal-dual solver (l1decode_pd, three coordinates batched:
the k_pd_* kernels and pd_solve of desc_amd/csrc/irls.hip, the per-element text and the scalar rules of irls_math.h).

  (a) a float64 NumPy restatement in the kernels' own order: the formulas of pd_*_at with their bracketing, pd_gather_row16's 16 lanes
      and butterfly, the partial reductions (thread t of block b takes the elements b * 256 + t + k * 65 536 in order, block_reduce's
      tree with strides 128 ... 1, then the host over the blocks 0 .. RG - 1: a sum from 0.0, fmin from +inf, fmax from 0; fmin / fmax
      skip NaN), the scalar rules, and pd_solve's loop with its per-coordinate run / search / accept handling.  The Newton solve is
      laa_maps_oracle.pcg_a(..., w3=True).  Every operation is + - * / sqrt fabs fmin fmax, correctly rounded on both sides: the
      device must return the same bits, so no decision of the loop hangs on the last place of a double.
  (b) ``*_b``: the formulas of one step in mpmath at 50 digits on the same doubles, to check (a)'s formulas independently.

Reference text restated (never copied): Utils/BoxMedianSO3Graph.m:245-360.  State arrays are (m, 3) per edge and (n, 3) per node, a
column per coordinate; edges 0-based, sorted, i < j; node 0 is grounded."""
import mpmath as mp
import numpy as np

from tests import laa_maps_oracle as O

RG = 256                                 # PD_RG: blocks of the partial-reduction kernels
SPAN = RG * 256                          # threads of such a launch: element e belongs to thread e % SPAN, pass e // SPAN
EDGE = ("y", "Ax", "u", "f1", "f2", "l1", "l2", "w2", "s1", "s2", "sx", "ev1", "ev2", "Adx", "du", "d1", "d2")
NODE = ("x", "Atv", "w1p", "dg", "dx", "Atdv")
TOL, ALPHA, BETA, MU, MAX_BACKITER = 2.220446049250313e-16, 0.01, 0.5, 10.0, 32
AGAIN, ACCEPT, STUCK = 0, 1, 2
F = np.float64
_quiet = O._quiet


# =================================================================================================== the graph
def csr(n, ii, jj):
    """The library's CSR as arrays (laa_maps_oracle.csr_rows is the same order as lists): row v holds the edges (i, v) in edge order
    with sign +1, then the edges (v, j) in edge order with sign -1.  -> rowptr (n + 1), eid, sgn."""
    ii = np.asarray(ii, dtype=np.int64); jj = np.asarray(jj, dtype=np.int64); m = len(ii)
    cl, cu = np.bincount(jj, minlength=n), np.bincount(ii, minlength=n)
    rowptr = np.concatenate([[0], np.cumsum(cl + cu)])
    eid = np.zeros(2 * m, dtype=np.int64); sgn = np.zeros(2 * m)
    lo, up = np.argsort(jj, kind="stable"), np.argsort(ii, kind="stable")
    ol, ou = np.concatenate([[0], np.cumsum(cl)])[:-1], np.concatenate([[0], np.cumsum(cu)])[:-1]
    pl = rowptr[jj[lo]] + (np.arange(m) - ol[jj[lo]])
    pu = rowptr[ii[up]] + cl[ii[up]] + (np.arange(m) - ou[ii[up]])
    eid[pl] = lo; sgn[pl] = 1.0; eid[pu] = up; sgn[pu] = -1.0
    return rowptr, eid, sgn


def blank(n, m):
    st = {k: np.zeros((m, 3)) for k in EDGE}
    st.update({k: np.zeros((n, 3)) for k in NODE})
    return st


def copy(st):
    return {k: v.copy() for k, v in st.items()}


# =================================================================================================== the reductions
def _tree(acc, op):
    """block_reduce over (SPAN, K) thread values: -> the raw partials (RG, K)."""
    sh = acc.reshape(RG, 256, -1).copy()
    st = 128
    while st > 0:
        sh[:, :st] = op(sh[:, :st], sh[:, st:2 * st])
        st >>= 1
    return sh[:, 0, :].copy()


def _fold(acc, items, op, first=0):
    """The grid-stride loop: thread e % SPAN takes element e (from `first` on) in the order of its passes; acc (SPAN, K) in place.
    items: the (vals, cond) a thread folds in at one element, in order; where cond (None: everywhere) is false the accumulator is left
    alone."""
    count = items[0][0].shape[0]
    for base in range(0, count, SPAN):
        lo = first if base == 0 else 0
        hi = min(SPAN, count - base)
        if lo >= hi:
            continue
        for vals, cond in items:
            new = op(acc[lo:hi], vals[base + lo:base + hi])
            acc[lo:hi] = new if cond is None else np.where(cond[base + lo:base + hi], new, acc[lo:hi])
    return acc


@_quiet
def host_sum(part):
    """read_part: the blocks in order from 0.0."""
    a = np.zeros(part.shape[1])
    for b in range(part.shape[0]):
        a = a + part[b]
    return a


@_quiet
def host_min(part):
    a = np.full(part.shape[1], np.inf)
    for b in range(part.shape[0]):
        a = np.fmin(a, part[b])
    return a


@_quiet
def host_max(part):
    a = np.zeros(part.shape[1])
    for b in range(part.shape[0]):
        a = np.fmax(a, part[b])
    return a


# =================================================================================================== the kernels
@_quiet
def absmax(st):
    """k_pd_absmax -> partials (RG, 3)."""
    acc = _fold(np.zeros((SPAN, 3)), [(np.abs(st["y"]), None)], np.fmax)
    return _tree(acc, np.fmax)


@_quiet
def init(st, ymax):
    """k_pd_init (pd_init_at): writes Ax, u, f1, f2, l1, l2, ev1 of every coordinate."""
    st = copy(st)
    yy = st["y"]; ax = np.zeros_like(yy)
    uu = 0.95 * np.abs(yy - ax) + 0.10 * np.asarray(ymax, dtype=F)[None, :]
    g1 = (ax - yy) - uu; g2 = (-ax + yy) - uu
    m1 = -1.0 / g1; m2 = -1.0 / g2
    st.update(Ax=ax, u=uu, f1=g1, f2=g2, l1=m1, l2=m2, ev1=m1 - m2)
    return st


@_quiet
def gather(n, C, ev1, ev2, mode, coef=(0.0, 0.0, 0.0)):
    """k_pd_gather<mode> (pd_gather_row16, pd_gather_out): lane l of 16 takes the row's slots l, l + 16, ... in order, then the
    butterfly.  Every row v < n is written; row 0 (grounded) gathers nothing: g = h = 0.  -> out (n, 3)."""
    rowptr, eid, sgn = C
    g = np.zeros((n, 3)); h = np.zeros((n, 3))
    deg = np.diff(rowptr); S = -(-deg // 16); S[0] = 0
    lane = np.arange(16)
    for sv in np.unique(S[S > 0]):
        rows = np.flatnonzero(S == sv)
        ag = np.zeros((rows.size, 16, 3)); ah = np.zeros((rows.size, 16, 3))
        for p in range(int(sv)):
            t = rowptr[rows][:, None] + 16 * p + lane[None, :]
            ok = t < rowptr[rows + 1][:, None]
            t = np.where(ok, t, 0)
            e = eid[t]
            sg = np.ones(t.shape) if mode == 2 else sgn[t]
            ag = np.where(ok[:, :, None], ag + sg[:, :, None] * ev1[e], ag)
            if mode == 1:
                ah = np.where(ok[:, :, None], ah + sg[:, :, None] * ev2[e], ah)
        g[rows] = O._tree16_rows(ag)
        if mode == 1:
            h[rows] = O._tree16_rows(ah)
    return np.asarray(coef, dtype=F)[None, :] * g - h if mode == 1 else g


@_quiet
def pre(st, tau, act):
    """k_pd_pre (pd_pre_at): w2, s1, s2, sx, ev1, ev2 of the coordinates in act; the others get sx = 1, ev1 = ev2 = 0 and keep the rest."""
    st = copy(st)
    for c in range(3):
        if not act[c]:
            st["sx"][:, c] = 1.0; st["ev1"][:, c] = 0.0; st["ev2"][:, c] = 0.0
            continue
        g1, g2, m1, m2 = st["f1"][:, c], st["f2"][:, c], st["l1"][:, c], st["l2"][:, c]
        it = F(1.0) / F(tau[c])
        ww = -1.0 - it * (1.0 / g1 + 1.0 / g2)
        a1 = -m1 / g1 - m2 / g2
        a2 = m1 / g1 - m2 / g2
        ax = a1 - a2 * a2 / a1
        st["w2"][:, c] = ww; st["s1"][:, c] = a1; st["s2"][:, c] = a2; st["sx"][:, c] = ax
        st["ev1"][:, c] = -1.0 / g1 + 1.0 / g2
        st["ev2"][:, c] = (a2 / a1) * ww
    return st


@_quiet
def direction(st, ii, jj, tau, act):
    """k_pd_dir (pd_dir_at): Adx, du, d1, d2, ev1 of the coordinates in act (the others: ev1 = 0 only), and the step-length minima as
    partials (RG, 6): the lamu bound per coordinate, then the fu bound."""
    st = copy(st)
    ii = np.asarray(ii, dtype=np.int64); jj = np.asarray(jj, dtype=np.int64); m = len(ii)
    acc = np.full((SPAN, 6), np.inf)
    for c in range(3):
        if not act[c]:
            st["ev1"][:, c] = 0.0
            continue
        dx = st["dx"][:, c]
        adx = np.where(jj > 0, dx[jj], 0.0) - np.where(ii > 0, dx[ii], 0.0)
        it = F(1.0) / F(tau[c])
        g1, g2, m1, m2 = st["f1"][:, c], st["f2"][:, c], st["l1"][:, c], st["l2"][:, c]
        dd = (st["w2"][:, c] - st["s2"][:, c] * adx) / st["s1"][:, c]
        q1 = -(m1 / g1) * (adx - dd) - m1 - it * 1.0 / g1
        q2 = (m2 / g2) * (adx + dd) - m2 - it * 1.0 / g2
        st["Adx"][:, c] = adx; st["du"][:, c] = dd; st["d1"][:, c] = q1; st["d2"][:, c] = q2; st["ev1"][:, c] = q1 - q2
        col = lambda v: v.reshape(m, 1)
        _fold(acc[:, c:c + 1], [(col(-m1 / q1), col(q1 < 0)), (col(-m2 / q2), col(q2 < 0))], np.fmin)
        _fold(acc[:, 3 + c:4 + c], [(col(-g1 / (adx - dd)), col((adx - dd) > 0)), (col(-g2 / (-adx - dd)), col((-adx - dd) > 0))], np.fmin)
    return st, _tree(acc, np.fmin)


@_quiet
def resid(st, tau, s, act, trial):
    """k_pd_resid<trial> (pd_resid_edge, pd_resid_node): |[rdual; rcent]|^2 per coordinate as partials (RG, 3); a thread adds its edge
    terms in pass order, then its node terms (node 0 has none); a coordinate not in act stays 0."""
    acc = np.zeros((SPAN, 3))
    m, n = st["y"].shape[0], st["x"].shape[0]
    for c in range(3):
        if not act[c]:
            continue
        y, Ax, uu, m1, m2 = (st[k][:, c] for k in ("y", "Ax", "u", "l1", "l2"))
        ax = Ax
        if trial:
            sc = F(s[c])
            uu = st["u"][:, c] + sc * st["du"][:, c]; ax = st["Ax"][:, c] + sc * st["Adx"][:, c]
            m1 = st["l1"][:, c] + sc * st["d1"][:, c]; m2 = st["l2"][:, c] + sc * st["d2"][:, c]
        g1 = (ax - y) - uu; g2 = (-ax + y) - uu
        it = F(1.0) / F(tau[c])
        rd = 1.0 + (-m1 - m2)
        r1 = -m1 * g1 - it; r2 = -m2 * g2 - it
        term = rd * rd + r1 * r1 + r2 * r2
        col = acc[:, c:c + 1]
        _fold(col, [(term.reshape(m, 1), None)], np.add)
        t = st["Atv"][:, c] + F(s[c]) * st["Atdv"][:, c] if trial else st["Atv"][:, c]
        _fold(col, [((t * t).reshape(n, 1), None)], np.add, first=1)
    return _tree(acc, np.add)


@_quiet
def accept(st, s, act):
    """k_pd_accept (pd_accept_at, pd_accept_node): the coordinates in act move u, Ax, l1, l2, f1, f2 and the rows 1.. of x and Atv; then
    fu1' lamu1 and fu2' lamu2 of every coordinate as partials (RG, 6)."""
    st = copy(st)
    m = st["y"].shape[0]
    for c in range(3):
        if not act[c]:
            continue
        sc = F(s[c]); y = st["y"][:, c]
        uu = st["u"][:, c] + sc * st["du"][:, c]; ax = st["Ax"][:, c] + sc * st["Adx"][:, c]
        m1 = st["l1"][:, c] + sc * st["d1"][:, c]; m2 = st["l2"][:, c] + sc * st["d2"][:, c]
        g1 = (ax - y) - uu; g2 = (-ax + y) - uu
        st["u"][:, c] = uu; st["Ax"][:, c] = ax; st["l1"][:, c] = m1; st["l2"][:, c] = m2; st["f1"][:, c] = g1; st["f2"][:, c] = g2
        st["x"][1:, c] = st["x"][1:, c] + sc * st["dx"][1:, c]
        st["Atv"][1:, c] = st["Atv"][1:, c] + sc * st["Atdv"][1:, c]
    acc = _fold(np.zeros((SPAN, 6)), [(np.concatenate([st["f1"] * st["l1"], st["f2"] * st["l2"]], axis=1), None)], np.add)
    return st, _tree(acc, np.add)


def stage(name, n, ii, jj, C, st, scal):
    """One launch as desc_test_irls_pd_stage makes it, on the snapshot st with scal = dict(tau, s, ymax, act): -> (state after, the
    partials (RG, K) or None).  gather1 forms its coefficient from tau and act as pd_solve does; gather2 takes no scalars."""
    tau, s, ymax, act = scal["tau"], scal["s"], scal["ymax"], scal["act"]
    if name == "absmax":
        return st, absmax(st)
    if name == "init":
        return init(st, ymax), None
    if name in ("gather0", "gather1", "gather2"):
        new = copy(st)
        if name == "gather0":
            new["Atv"] = gather(n, C, st["ev1"], None, 0)
        elif name == "gather1":
            new["w1p"] = gather(n, C, st["ev1"], st["ev2"], 1, [pd_gather_coef(act[c], tau[c]) for c in range(3)])
        else:
            new["dg"] = gather(n, C, st["sx"], None, 2)
        return new, None
    if name == "pre":
        return pre(st, tau, act), None
    if name == "dir":
        return direction(st, ii, jj, tau, act)
    if name in ("resid", "resid_trial"):
        return st, resid(st, tau, s, act, name == "resid_trial")
    if name == "accept":
        return accept(st, s, act)
    raise ValueError(name)


def raw_part(part_in, partials):
    """The 6 * RG doubles of the partials buffer after a launch that found part_in there: [RG][K] from its start, the rest untouched."""
    out = np.asarray(part_in, dtype=F).reshape(-1).copy()
    if partials is not None:
        out[:partials.size] = partials.reshape(-1)
    return out


# =================================================================================================== the scalar rules (irls_math.h)
@_quiet
def pd_sdg(d1, d2):
    return -(F(d1) + F(d2))


@_quiet
def pd_tau(M, sdg):
    return F(MU) * F(2.0) * F(M) / F(sdg)


@_quiet
def pd_goes_on(sdg, pditer, pdmaxiter):
    return int(not (bool(F(sdg) < TOL) or pditer >= pdmaxiter))


@_quiet
def pd_gather_coef(run, tau):
    return F(-1.0) / F(tau) if run else F(0.0)


@_quiet
def pd_step_length(mn_lam, mn_fu):
    s = np.fmin(F(1.0), F(mn_lam))
    return F(0.99) * np.fmin(s, F(mn_fu))


@_quiet
def pd_trial(rr, resnorm, s, backiter):
    """-> (verdict, the halved s, backiter + 1, the s tried)."""
    suffdec = bool(np.sqrt(F(rr)) <= (F(1.0) - F(ALPHA) * F(s)) * F(resnorm))
    tried = F(s); s = F(BETA) * F(s); backiter += 1
    if backiter > MAX_BACKITER:
        return STUCK, s, backiter, tried
    return (ACCEPT if suffdec else AGAIN), s, backiter, tried


# =================================================================================================== pd_solve
@_quiet
def solve(n, ii, jj, B, pdmaxiter, watch=None):
    """pd_solve on B (m, 3) from x = 0.  -> dict(x, u, l1, l2, Ax, Atv, steps, ill, stuck, solves, cg_total, cg_unconverged, cap_steps (the steps whose CG stopped at its cap), trace
    (records, 3, 8): per step (record 0: the start) and coordinate {takes part, the CG's bad, first trial step, trials, verdict, sdg, tau,
    resnorm after the step}, state: every array at the end).  watch(step, stage, before, scal, after, part): called around every
    kernel of the loop with the state before and after it, scal = dict(tau, s, ymax, act) of the launch, part the raw partials."""
    ii = np.asarray(ii, dtype=np.int64); jj = np.asarray(jj, dtype=np.int64)
    B = np.asarray(B, dtype=F).reshape(-1, 3); m = B.shape[0]; Mf = F(m)
    C = csr(n, ii, jj)
    st = blank(n, m); st["y"] = B.copy()
    one, zero3 = (1, 1, 1), np.zeros(3)
    step = 0

    def saw(stage, before, after, part=None, tau=zero3, s=zero3, ymax=zero3, act=one):
        if watch is not None:
            watch(step, stage, before, dict(tau=np.array(tau, dtype=F), s=np.array(s, dtype=F), ymax=np.array(ymax, dtype=F), act=tuple(int(a) for a in act)),
                  after, part)

    part = absmax(st); saw("absmax", st, st, part)
    ymax = host_max(part)
    new = init(st, ymax); saw("init", st, new, ymax=ymax); st = new
    new = copy(st); new["Atv"] = gather(n, C, st["ev1"], None, 0); saw("gather0", st, new); st = new
    tau = np.zeros(3); resnorm = np.zeros(3); sdg = np.zeros(3)
    out = dict(steps=0, ill=0, stuck=0, solves=0, cg_total=0, cg_unconverged=0, cap_steps=[])
    trace = []

    def scalars(act, dots_part):
        dots = host_sum(dots_part)
        b_tau = np.zeros(3); b_act = [0, 0, 0]
        for c in range(3):
            if act[c]:
                sdg[c] = pd_sdg(dots[c], dots[3 + c]); tau[c] = pd_tau(Mf, sdg[c]); b_act[c] = 1; b_tau[c] = tau[c]
        p = resid(st, b_tau, zero3, b_act, False); saw("resid", st, st, p, tau=b_tau, act=b_act)
        rr = host_sum(p)
        for c in range(3):
            if act[c]:
                resnorm[c] = np.sqrt(rr[c])

    def close(rec):
        for c in range(3):
            rec[c, 5:8] = sdg[c], tau[c], resnorm[c]
        trace.append(rec)

    run = [1, 1, 1]
    new, part = accept(st, zero3, (0, 0, 0)); saw("accept", st, new, part, act=(0, 0, 0)); st = new
    scalars(run, part)
    rec = np.zeros((3, 8)); rec[:, 0] = 1.0; close(rec)
    run = [pd_goes_on(sdg[c], step, pdmaxiter) for c in range(3)]
    while any(run):
        step += 1
        rec = np.zeros((3, 8)); rec[:, 0] = run
        a_act = list(run)
        new = pre(st, tau, a_act); saw("pre", st, new, tau=tau, act=a_act); st = new
        coef = [pd_gather_coef(run[c], tau[c]) for c in range(3)]
        new = copy(st); new["w1p"] = gather(n, C, st["ev1"], st["ev2"], 1, coef); saw("gather1", st, new, tau=tau, act=a_act); st = new
        new = copy(st); new["dg"] = gather(n, C, st["sx"], None, 2); saw("gather2", st, new); st = new
        out["solves"] += 1
        ref = O.pcg_a(n, ii, jj, st["sx"], st["w1p"], st["dg"], act=tuple(run), w3=True)
        st["dx"] = ref["x"].copy()
        out["cg_total"] += ref["total"]; out["cg_unconverged"] += ref["unconverged"]
        if ref["unconverged"]:
            out["cap_steps"].append(step)
        for c in range(3):
            if ref["bad"][c]:
                out["ill"] += 1; run[c] = 0; a_act[c] = 0; rec[c, 1] = 1.0
        if not any(run):
            close(rec)
            break
        out["steps"] += sum(run)
        new, part = direction(st, ii, jj, tau, a_act); saw("dir", st, new, part, tau=tau, act=a_act); st = new
        mins = host_min(part)
        new = copy(st); new["Atdv"] = gather(n, C, st["ev1"], None, 0)
        s = np.zeros(3)
        for c in range(3):
            if run[c]:
                s[c] = pd_step_length(mins[c], mins[3 + c]); rec[c, 2] = s[c]
        st = new
        search = list(run); backiter = [0, 0, 0]; acc = [0, 0, 0]; s_acc = np.zeros(3)
        while any(search):
            p = resid(st, tau, s, search, True); saw("resid_trial", st, st, p, tau=tau, s=s, act=search)
            rr = host_sum(p)
            for c in range(3):
                if not search[c]:
                    continue
                verdict, s[c], backiter[c], tried = pd_trial(rr[c], resnorm[c], s[c], backiter[c])
                if verdict == STUCK:
                    out["stuck"] += 1; search[c] = 0; run[c] = 0
                elif verdict == ACCEPT:
                    search[c] = 0; acc[c] = 1; s_acc[c] = tried
                rec[c, 3] = backiter[c]; rec[c, 4] = verdict
        new, part = accept(st, s_acc, acc); saw("accept", st, new, part, s=s_acc, act=acc); st = new
        scalars(acc, part)
        for c in range(3):
            if acc[c]:
                run[c] = pd_goes_on(sdg[c], step, pdmaxiter)
        close(rec)
    out.update(x=st["x"], u=st["u"], l1=st["l1"], l2=st["l2"], Ax=st["Ax"], Atv=st["Atv"], trace=np.array(trace), state=st)
    return out


# =================================================================================================== (b): one step at 50 digits
def _m(a):
    return O.M(a)


def _bad(*v):
    return any(mp.isnan(t) or mp.isinf(t) for t in v)


def pre_b(st, tau):
    """pd_pre_at's formulas (BoxMedianSO3Graph.m:296-304) in mpf on the doubles of st: -> dict of (m, 3) mpf arrays w2 s1 s2 sx ev1 ev2
    and `mag`, the float magnitudes the roundings of (a) scale with."""
    f1, f2, l1, l2 = (_m(st[k]) for k in ("f1", "f2", "l1", "l2"))
    out = {k: np.empty(f1.shape, dtype=object) for k in ("w2", "s1", "s2", "sx", "ev1", "ev2")}
    mag = {k: np.zeros(f1.shape) for k in out}
    for (e, c), g1 in np.ndenumerate(f1):
        g2, m1, m2 = f2[e, c], l1[e, c], l2[e, c]
        it = 1 / mp.mpf(float(tau[c]))
        if _bad(g1, g2, m1, m2, it) or g1 == 0 or g2 == 0:
            for k in out: out[k][e, c] = mp.nan
            continue
        ww = -1 - it * (1 / g1 + 1 / g2)
        a1 = -m1 / g1 - m2 / g2
        a2 = m1 / g1 - m2 / g2
        big = abs(m1 / g1) + abs(m2 / g2)
        vals = dict(w2=ww, s1=a1, s2=a2, sx=(a1 - a2 * a2 / a1) if a1 != 0 else mp.nan, ev1=-1 / g1 + 1 / g2,
                    ev2=(a2 / a1) * ww if a1 != 0 else mp.nan)
        mags = dict(w2=1 + abs(it) * (abs(1 / g1) + abs(1 / g2)), s1=big, s2=big, sx=big + (big * big / abs(a1) if a1 != 0 else 0),
                    ev1=abs(1 / g1) + abs(1 / g2), ev2=(big / abs(a1) if a1 != 0 else 0) * (1 + abs(it) * (abs(1 / g1) + abs(1 / g2))))
        for k in out:
            out[k][e, c] = vals[k]; mag[k][e, c] = float(mags[k])
    return out, mag


def direction_b(st, ii, jj, tau):
    """pd_dir_at's formulas (:315-324) in mpf from the doubles of st (dx, w2, s1, s2 included): Adx du d1 d2 and their magnitudes."""
    f1, f2, l1, l2, w2, s1, s2, dx = (_m(st[k]) for k in ("f1", "f2", "l1", "l2", "w2", "s1", "s2", "dx"))
    out = {k: np.empty(f1.shape, dtype=object) for k in ("Adx", "du", "d1", "d2")}
    mag = {k: np.zeros(f1.shape) for k in out}
    for (e, c), g1 in np.ndenumerate(f1):
        g2, m1, m2 = f2[e, c], l1[e, c], l2[e, c]
        it = 1 / mp.mpf(float(tau[c]))
        xj = dx[jj[e], c] if jj[e] > 0 else mp.mpf(0)
        xi = dx[ii[e], c] if ii[e] > 0 else mp.mpf(0)
        if _bad(g1, g2, m1, m2, it, xi, xj, w2[e, c], s1[e, c], s2[e, c]) or g1 == 0 or g2 == 0 or s1[e, c] == 0:
            for k in out: out[k][e, c] = mp.nan
            continue
        adx = xj - xi
        dd = (w2[e, c] - s2[e, c] * adx) / s1[e, c]
        mdd = (abs(w2[e, c]) + abs(s2[e, c] * adx)) / abs(s1[e, c])
        span = abs(xj) + abs(xi) + mdd
        vals = dict(Adx=adx, du=dd, d1=-(m1 / g1) * (adx - dd) - m1 - it / g1, d2=(m2 / g2) * (adx + dd) - m2 - it / g2)
        mags = dict(Adx=abs(xj) + abs(xi), du=mdd, d1=abs(m1 / g1) * span + abs(m1) + abs(it / g1), d2=abs(m2 / g2) * span + abs(m2) + abs(it / g2))
        for k in out:
            out[k][e, c] = vals[k]; mag[k][e, c] = float(mags[k])
    return out, mag


def resid_b(st, tau, s, trial):
    """|[rdual; rcent]|^2 per coordinate (:280-283, :334-336) summed in mpf: -> 3 mpf, and the sums of the terms' magnitudes (float)."""
    tot, mags = [], []
    m, n = st["y"].shape[0], st["x"].shape[0]
    for c in range(3):
        it = 1 / mp.mpf(float(tau[c])); sc = mp.mpf(float(s[c])) if trial else mp.mpf(0)
        acc = mp.mpf(0); big = mp.mpf(0)
        for e in range(m):
            y, ax, uu, m1, m2 = (mp.mpf(float(st[k][e, c])) for k in ("y", "Ax", "u", "l1", "l2"))
            if trial:
                ax += sc * mp.mpf(float(st["Adx"][e, c])); uu += sc * mp.mpf(float(st["du"][e, c]))
                m1 += sc * mp.mpf(float(st["d1"][e, c])); m2 += sc * mp.mpf(float(st["d2"][e, c]))
            g1 = ax - y - uu; g2 = -ax + y - uu
            acc += (1 - m1 - m2) ** 2 + (-m1 * g1 - it) ** 2 + (-m2 * g2 - it) ** 2
            big += (1 + abs(m1) + abs(m2)) ** 2 + (abs(m1 * g1) + abs(it)) ** 2 + (abs(m2 * g2) + abs(it)) ** 2
        for v in range(1, n):
            t = mp.mpf(float(st["Atv"][v, c])) + sc * mp.mpf(float(st["Atdv"][v, c]))
            acc += t * t; big += (abs(mp.mpf(float(st["Atv"][v, c]))) + abs(sc * mp.mpf(float(st["Atdv"][v, c])))) ** 2
        tot.append(acc); mags.append(float(big))
    return tot, mags

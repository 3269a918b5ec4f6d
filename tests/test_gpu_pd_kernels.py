"""The eight kernels of the L1 stage's primal-dual solver (desc_amd/csrc/irls.hip: k_pd_absmax, k_pd_init, k_pd_gather<0|1|2>, k_pd_pre,
k_pd_dir, k_pd_resid<false|true>, k_pd_accept) one launch at a time, through desc_test_irls_pd_stage: the hook uploads a snapshot of the
solver's whole state, launches one kernel with the grid pd_solve uses (egrid, rgrid, RG) and returns every array and the raw [RG][K]
partials.

Comparison rule: every array and every raw partial is bit-equal to restatement (a) of tests/pd_oracle.py (NaN positions and the signs of
zeros and infinities included).  Arrays the kernel does not write must come back with the bits they went in with, and the part of the
partials buffer behind [RG][K] too: the comparison runs over all 17 + 6 arrays and all 6 * 256 partials of every launch.

Case -> line reached
  a single edge (n = 2)                                 one thread with work; k_pd_gather's group of four rows with three idle
  paths with m = 255, 256, 257                          the last thread of block 0 / the first of block 1 of every edge loop
  stars of 15, 16, 17, 33 spokes, hub 0 and hub last    pd_gather_row16: one, two and three passes of the 16-lane row loop, a partial
                                                        last pass; hub 0: the grounded row gathers nothing and is written as 0
  n = 3, 4, 5, 17                                       k_pd_gather's groups of four rows: v >= n inside the last group
  complete graph on 363 nodes, m = 65 703               the second grid-stride pass of every RG kernel's edge loop (167 threads)
  wheel of 65 600 nodes, hub last, m = 131 198          the second pass of the node loops of k_pd_resid / k_pd_accept (64 threads), of
                                                        k_pd_gather's row loop (rgrid = 2048: 32 768 rows a pass) and a third pass of the
                                                        edge loops; the hub row has 65 599 slots (4100 passes of the lane loop)
  states                                                (a)'s state before every launch of steps 0, 1 and 5 of a solve on the shape
                                                        itself (n <= 40), and synthetic finite data of mixed sign over six decades
                                                        on every shape (the only data of the large ones)
  masks                                                 the eight act combinations on n = 17 for pre, dir, resid, resid_trial, accept
  non-finite                                            a zero coordinate of y, NaN in y (absmax), no candidate / NaN candidates
                                                        (dir), a NaN coordinate next to two finite ones (resid, accept)
  left out                                              egrid's own cap of 2048 blocks (m > 524 288): the snapshot of such a graph is
                                                        0.2 GB a call, and the loop it wraps is the one the wheel wraps three times

Measured on an MI355X: every launch bit-equal to (a) in all 23 arrays and all 1536 partials: 10 stages on 18 shapes with synthetic
data (the wheel: 1.0 s for its ten launches with their 53 MB snapshots, the complete graph 0.4 s, the others under 0.1 s), the 19
launches of steps 0, 1 and 5 of an 18-step solve on each of the 13 small shapes, 5 x 8 mask combinations, and the non-finite cases: ymax = 0 for
a zero coordinate and u = 0, lamu = -inf, ev = NaN from it; NaN skipped by the maxima; +inf partials where no candidate exists; NaN
candidates skipped among finite ones; a NaN coordinate leaves the other two coordinates' partials their bits.
Found and fixed through test_act_masks[accept]: k_pd_accept wrote row 0 of x and Atv (x + s * dx with dx(0) = 0 in the solver, so no
result changed); it now leaves the grounded row alone, as k_pd_resid does.  Every test prints what it ran (-s)."""
import numpy as np
import pytest

from tests import laa_maps_cases as K
from tests import laa_maps_oracle as O
from tests import pd_cases as PC
from tests import pd_oracle as P

pytestmark = pytest.mark.gpu

_dev = {}


def device_problem(lib, name):
    if name not in _dev:
        n, ii, jj = PC.stage_shapes()[name]
        _dev[name] = (lib.DeviceProblem(lib.ProblemArrays(n, ii.astype(np.int32), jj.astype(np.int32), K.identity_rij(len(ii)))), P.csr(n, ii, jj))
    return _dev[name]


def sentinel_part():
    return 7.25 + np.arange(6 * P.RG, dtype=np.float64)


def check_stage(lib, name, stage, st, scal, tag=""):
    """One launch against (a): -> (device state, device raw partials, reference state, reference partials or None)."""
    n, ii, jj = PC.stage_shapes()[name]
    dp, C = device_problem(lib, name)
    part_in = sentinel_part()
    got, gpart = lib.hook_pd_stage(dp, stage, st, part_in, tau=scal["tau"], s=scal["s"], ymax=scal["ymax"], act=scal["act"])
    want, wpart = P.stage(stage, n, ii, jj, C, st, scal)
    changed = [k for k in want if not O.bit_equal(want[k], st[k])]
    for k in P.EDGE + P.NODE:
        assert O.bit_equal(got[k], want[k]), f"{name} {stage} {tag}: {k} differs from (a) at {np.argwhere(~_same(got[k], want[k]))[:4].tolist()}"
    assert O.bit_equal(gpart, P.raw_part(part_in, wpart)), f"{name} {stage} {tag}: raw partials differ from (a)"
    return got, gpart, want, wpart, changed


def _same(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return (na & nb) | (~na & ~nb & (a.view(np.uint64) == b.view(np.uint64)))


WRITES = dict(absmax=set(), init={"Ax", "u", "f1", "f2", "l1", "l2", "ev1"}, gather0={"Atv"}, gather1={"w1p"}, gather2={"dg"},
              pre={"w2", "s1", "s2", "sx", "ev1", "ev2"}, dir={"Adx", "du", "d1", "d2", "ev1"}, resid=set(), resid_trial=set(),
              accept={"Ax", "u", "l1", "l2", "f1", "f2", "x", "Atv"})
SHAPES = ("edge", "path255", "path256", "path257", "star15-hub0", "star15-hub-last", "star16-hub0", "star16-hub-last", "star17-hub0",
          "star17-hub-last", "star33-hub0", "star33-hub-last", "n3", "n4", "n5", "n17", "k363", "wheel65600")


@pytest.mark.parametrize("name", SHAPES)
def test_every_stage_on_synthetic_state(lib, name):
    n, ii, jj = PC.stage_shapes()[name]
    st, scal = PC.synthetic_state(n, len(ii), seed=SHAPES.index(name))
    for stage in lib.PD_STAGES:
        got, gpart, want, wpart, changed = check_stage(lib, name, stage, st, scal)
        assert set(changed) <= WRITES[stage], (stage, changed)
    passes = dict(edge=-(-len(ii) // P.SPAN), node=-(-n // P.SPAN), rows=-(-n // 32768))
    print(f"[pd kernels] {name}: n={n} m={len(ii)} passes={passes}, all {len(lib.PD_STAGES)} stages bit-equal on synthetic data")
    if name == "k363":
        assert passes["edge"] == 2
    if name == "wheel65600":
        assert passes == dict(edge=3, node=2, rows=3) and np.diff(P.csr(n, ii, jj)[0]).max() == 65599


LARGE = ("path255", "path256", "path257", "k363", "wheel65600")


@pytest.mark.parametrize("name", [s for s in SHAPES if s not in LARGE])
def test_every_stage_on_the_states_of_a_solve(lib, name):
    """(a)'s own state before the first launch of every stage in steps 0, 1 and 5 of a solve on this graph."""
    n, ii, jj = PC.stage_shapes()[name]
    g = np.random.default_rng(100 + SHAPES.index(name))
    B = g.normal(size=(len(ii), 3)) * 0.3
    seen = {}

    def watch(step, stage, before, scal, after, part):
        if step in (0, 1, 5) and (step, stage) not in seen:
            seen[(step, stage)] = (P.copy(before), scal)
    res = P.solve(n, ii, jj, B, 6, watch=watch)
    for (step, stage), (before, scal) in sorted(seen.items()):
        check_stage(lib, name, stage, before, scal, tag=f"step {step}")
    stages = {s for _, s in seen}
    print(f"[pd kernels] {name}: {len(seen)} launches of steps {sorted({k for k, _ in seen})} bit-equal; the solve took {res['steps']} steps, ill {res['ill']}, stuck {res['stuck']}")
    assert {"absmax", "init", "gather0", "accept", "resid"} <= stages
    if res["steps"]:
        assert {"pre", "gather1", "gather2", "dir", "resid_trial"} <= stages


@pytest.mark.parametrize("stage", ["pre", "dir", "resid", "resid_trial", "accept"])
def test_act_masks(lib, stage):
    """All eight act combinations on n = 17: a coordinate not in act keeps every bit of its columns, except what the kernels document
    (pre: sx = 1, ev1 = ev2 = 0; dir: ev1 = 0), its partials stay at the neutral value (resid: 0, dir: +inf), and row 0 of every node
    array is untouched (the synthetic state has a non-zero row 0 in dx and Atdv, so a write would show)."""
    name = "n17"
    n, ii, jj = PC.stage_shapes()[name]
    st, scal = PC.synthetic_state(n, len(ii), seed=77)
    assert np.all(st["dx"][0] != 0) and np.all(st["Atdv"][0] != 0)
    for mask in range(8):
        act = tuple((mask >> c) & 1 for c in range(3))
        got, gpart, want, wpart, _ = check_stage(lib, name, stage, st, dict(scal, act=act), tag=f"act {act}")
        for k in P.NODE:
            assert O.bit_equal(got[k][0], st[k][0]), (stage, act, k)
        part = None if wpart is None else gpart[:wpart.size].reshape(wpart.shape)
        for c in range(3):
            if act[c]:
                if WRITES[stage]:
                    assert any(not O.bit_equal(got[k][:, c], st[k][:, c]) for k in WRITES[stage]), (stage, act, c)
                continue
            for k in P.EDGE + P.NODE:
                if stage == "pre" and k in ("sx", "ev1", "ev2"):
                    assert np.all(got[k][:, c] == (1.0 if k == "sx" else 0.0)) and not np.signbit(got[k][:, c]).any()
                elif stage == "dir" and k == "ev1":
                    assert np.all(got[k][:, c] == 0.0) and not np.signbit(got[k][:, c]).any()
                else:
                    assert O.bit_equal(got[k][:, c], st[k][:, c]), (stage, act, k, c)
            if stage in ("resid", "resid_trial"):
                assert np.all(part[:, c] == 0.0)
            if stage == "dir":
                assert np.all(part[:, c] == np.inf) and np.all(part[:, 3 + c] == np.inf)
    print(f"[pd kernels] masks: {stage} bit-equal under the 8 act combinations, inactive columns and row 0 untouched")


def test_absmax_and_init_with_a_zero_coordinate_and_nan(lib):
    name = "path257"
    n, ii, jj = PC.stage_shapes()[name]
    st, scal = PC.synthetic_state(n, len(ii), seed=5)
    st["y"][:, 1] = 0.0
    st["y"][::7, 0] = np.nan                                    # skipped by fmax, as by MATLAB's max
    st["y"][:, 2] = np.nan; st["y"][200, 2] = -3.5              # one finite value among NaN: thread 200 alone holds a maximum
    _, gpart, _, wpart, _ = check_stage(lib, name, "absmax", st, scal)
    ymax = P.host_max(gpart[:3 * P.RG].reshape(P.RG, 3))
    assert ymax[1] == 0.0 and ymax[0] == np.nanmax(np.abs(st["y"][:, 0])) and ymax[2] == 3.5
    got, _, _, _, _ = check_stage(lib, name, "init", st, dict(scal, ymax=ymax))
    assert np.all(got["u"][:, 1] == 0) and np.all(np.isinf(got["l1"][:, 1])) and np.all(np.isnan(got["ev1"][:, 1]))      # -1/-0 - -1/-0: inf - inf
    allnan = P.blank(n, len(ii)); allnan["y"][:] = np.nan
    _, gpart, _, _, _ = check_stage(lib, name, "absmax", allnan, scal)
    assert np.all(gpart[:3 * P.RG] == 0.0)
    print(f"[pd kernels] absmax: ymax = {ymax.tolist()} with a zero coordinate, NaN every 7th edge, one finite value among NaN; all NaN -> 0")


def test_dir_without_candidates_and_with_nan_candidates(lib):
    name = "n17"
    n, ii, jj = PC.stage_shapes()[name]
    st, scal = PC.synthetic_state(n, len(ii), seed=9)
    tau = scal["tau"].copy()
    # coordinate 0: dx = 0 and w2 > 0 give Adx - du < 0 and -Adx - du < 0; a tiny tau makes dlamu1, dlamu2 > 0: no candidate at all
    st["dx"][:, 0] = 0.0; st["w2"][:, 0] = np.abs(st["w2"][:, 0]); st["s2"][:, 0] = 0.0; tau[0] = 1e-12
    # coordinate 1: fu1 = NaN on every third edge: the fu candidates there are NaN (Adx - du does not depend on fu1)
    st["f1"][::3, 1] = np.nan
    got, gpart, want, wpart, _ = check_stage(lib, name, "dir", st, dict(scal, tau=tau))
    part = gpart[:6 * P.RG].reshape(P.RG, 6)
    assert np.all(part[:, 0] == np.inf) and np.all(part[:, 3] == np.inf)
    assert np.all(want["d1"][:, 0] > 0) and np.all(want["d2"][:, 0] > 0)
    d = want["Adx"][:, 1] - want["du"][:, 1]
    nan_cands = int(((d > 0) & np.isnan(st["f1"][:, 1])).sum()); fin_cands = int(((d > 0) & ~np.isnan(st["f1"][:, 1])).sum())
    assert nan_cands >= 1 and fin_cands >= 1
    mins = P.host_min(part)
    e = -want["Adx"][:, 1] - want["du"][:, 1]
    with np.errstate(all="ignore"):
        cands = np.concatenate([(-st["f1"][:, 1] / d)[d > 0], (-st["f2"][:, 1] / e)[e > 0]])
    assert np.isfinite(mins[4]) and mins[4] == np.nanmin(cands)                  # MATLAB's min over the candidates of :327-330
    print(f"[pd kernels] dir: coordinate 0 without a candidate: partials +inf; coordinate 1: {nan_cands} NaN candidates skipped among {fin_cands} finite ones, min = {mins[4]:.6g}")


@pytest.mark.parametrize("stage", ["resid", "resid_trial", "accept"])
def test_a_nan_coordinate_leaves_the_others_their_bits(lib, stage):
    name = "path257"
    n, ii, jj = PC.stage_shapes()[name]
    st, scal = PC.synthetic_state(n, len(ii), seed=13)
    _, clean, _, wclean, _ = check_stage(lib, name, stage, st, scal)
    bad = P.copy(st)
    for k in P.EDGE + P.NODE:
        bad[k][:, 1] = np.nan
    got, dirty, _, wdirty, _ = check_stage(lib, name, stage, bad, scal)
    K_ = wclean.shape[1]
    a, b = clean[:K_ * P.RG].reshape(P.RG, K_), dirty[:K_ * P.RG].reshape(P.RG, K_)
    used = (len(ii) + 255) // 256
    for col in range(K_):
        if col % 3 == 1:
            assert np.all(np.isnan(b[:used, col]))
        else:
            assert O.bit_equal(a[:, col], b[:, col]) and np.all(np.isfinite(b[:, col]))
    print(f"[pd kernels] {stage}: NaN in coordinate 1 reaches only its own partials ({used} blocks); coordinates 0 and 2 keep their bits")

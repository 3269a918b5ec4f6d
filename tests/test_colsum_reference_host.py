"""CPU tests of the integer reference of the mirror column sums (tests/colsum_cases.py) and of the reasons each case is in its table:
no GPU.  tests/test_gpu_colsum.py compares k_colsum_node with this reference bit for bit."""
import numpy as np
import pytest

from tests import colsum_cases as CC

HOST_CASES = ["triangle", "K64", "er40", "er200", "er60_full", "er150_full", "bridged150_60"]
_runs = {}


def _oracle_weights(oracle, case, state):
    """The oracle's weights of a state, computed once."""
    key = (case, state)
    if key not in _runs:
        nn, ii, jj, rij = CC.graph(case)
        st = CC.structure(oracle, case)
        step = CC.step_of(case, state)
        S0 = oracle.cycle_d(ii, jj, rij.reshape(-1, 9), st)
        res = oracle.pgd_run(st, S0, step["iters"], lr=step["lr"])
        assert res["iters_run"] == step["iters"]                   # the stop rule did not fire
        _runs[key] = res["w"]
    return _runs[key]


@pytest.mark.parametrize("state", sorted(CC.STATES))
@pytest.mark.parametrize("case", HOST_CASES)
def test_integer_reference_against_double_sums(oracle, case, state):
    """T_int * 2^-fx_bits against np.bincount(seg, w[mirror]) in doubles.  A term is rounded once, by at most 2^-(fx_bits + 1); the double
    sum of k non-negative terms is off by at most k eps times itself: |T_int 2^-fx - T_double| <= k 2^-(fx_bits + 1) + k eps T_double."""
    nn, ii, jj, rij = CC.graph(case)
    st = CC.structure(oracle, case)
    w = _oracle_weights(oracle, case, state)
    assert w.min() >= 0.0 and w.max() <= 1.0
    if state == "uniform":
        assert np.array_equal(w, CC.uniform_weights(st))           # what the GPU test uses without a download
    fx = CC.fx_bits_of(CC.max_degree(nn, ii, jj))
    q = CC.quantize(w, fx)
    assert np.all(np.abs(np.ldexp(q.astype(np.float64), -fx) - w) <= 2.0 ** -(fx + 1)) and q.min() >= 0
    seg = CC.seg_of_cycle(st)
    eps = np.finfo(np.float64).eps
    for T_int, key, k in zip(CC.mirror_sums(st, q), ("ikj", "jki"), CC.mirror_counts(st)):
        idx = np.asarray(st[key])
        ok = idx >= 0
        T_double = np.bincount(seg[ok], w[idx[ok]], minlength=st["m_pos"])
        assert T_int.max() < 2 ** 62 and T_int.min() >= 0
        bound = k * 2.0 ** -(fx + 1) + k * eps * T_double
        # (with eps = 2^-52 = 2 u the bound has room for the one further rounding of int64 -> double: (k - 1) u T for the sum + u T for it <= k eps T)
        assert np.all(np.abs(np.ldexp(T_int.astype(np.float64), -fx) - T_double) <= bound), (case, state, key)
        assert np.all(T_int[k == 0] == 0)
    # one rank's partial sums add up to the total for any split of the segments
    owned = np.arange(st["m_pos"]) % 3 == 1
    for tot, a, b in zip(CC.mirror_sums(st, q), CC.mirror_sums(st, q, owned), CC.mirror_sums(st, q, ~owned)):
        assert np.array_equal(a + b, tot)


def test_distinct_state_distinguishes_the_cycles_of_a_segment(oracle):
    """The condition the GPU test asserts on the downloaded weights, here on the oracle's: >= 99 % of the contributing cycles carry a
    weight of their own inside their segment -- so a column index paired with the wrong cycle of the same segment changes T."""
    for case in HOST_CASES:
        st = CC.structure(oracle, case)
        f = CC.distinct_fraction(st, _oracle_weights(oracle, case, "distinct"))
        print("%s: %.4f %% of the contributing cycles distinguishable" % (case, 100 * f))
        assert f >= 0.99, (case, f)
        if case != "triangle":                                     # one cycle per segment: trivially distinct
            assert CC.distinct_fraction(st, CC.uniform_weights(st)) < 0.5, case       # ... which the uniform state cannot offer


def test_fixed_point_position():
    assert [CC.fx_bits_of(d) for d in (1, 2, 3, 4, 62, 63, 64, 255, 256, 257, 1499, 32767)] == [61, 60, 60, 59, 56, 56, 55, 54, 53, 53, 51, 47]
    # half to even, as __double2ll_rn: 2.5 -> 2, 3.5 -> 4, 0.5 -> 0
    assert CC.quantize(np.array([2.5, 3.5, 0.5, 1.0]) * 2.0 ** -51, 51).tolist() == [2, 4, 0, 1]
    assert CC.quantize(np.array([1.0, 1.0 / 3.0]), 60).tolist() == [1 << 60, 384307168202282304]    # 1/3 in double * 2^60 is an integer: exact


def test_where_the_rounding_mode_shows(oracle):
    """w 2^fx_bits has a fractional part only where w < 2^(52 - fx_bits): the `uniform` state tells round-to-nearest from truncation and
    half-to-even from half-away only on some cases.  Which ones, so that nobody counts on the others for it."""
    seen = {}
    for case in HOST_CASES + ["hub1500_mid"]:
        nn, ii, jj, rij = CC.graph(case)
        st = CC.structure(oracle, case)
        fx = CC.fx_bits_of(CC.max_degree(nn, ii, jj))
        x = np.ldexp(CC.uniform_weights(st)[CC.contributing(st)], fx)
        fr = x - np.floor(x)
        seen[case] = (int(np.count_nonzero(fr)), int(np.count_nonzero(fr == 0.5)), int(np.count_nonzero(fr > 0.5)), x.size)
    for case in ("triangle", "K64", "er40", "er200"):             # 2^fx_bits / cnt is an integer for every count of these: blind to the rounding
        assert seen[case][0] == 0, (case, seen[case])
    assert seen["er150_full"][2] == seen["er150_full"][3]          # 2^54 / 100: truncation is off by one unit in EVERY term
    assert seen["hub1500_mid"][2] > 10000 and seen["er60_full"][2] > 20000
    assert seen["er60_full"][1] > 2000 and seen["bridged150_60"][1] > 1000       # exact halves: half-to-even against half-away-from-zero


def _facts(oracle, case):
    nn, ii, jj, rij = CC.graph(case)
    st = CC.structure(oracle, case)
    a, b = CC.mirror_counts(st)
    return dict(nn=nn, m=ii.shape[0], m_pos=st["m_pos"], max_deg=CC.max_degree(nn, ii, jj), cnt=np.diff(st["cum_ind"]), nact=np.concatenate([a, b]),
                nact_seg=np.maximum(a, b), avg_run=(a.sum() + b.sum()) / (2.0 * st["m_pos"]),
                sampled=float(np.mean(np.concatenate([st["ikj"], st["jki"]]) >= 0)))


def test_structural_claims_of_the_case_table(oracle):
    """Why each case is in CC.CASES (avg_run <= 10.5 selects the 8-lane instance, setup_node; a segment end of nact contributing cycles takes
    ceil(nact / (2 lanes)) rounds of colsum_walk)."""
    f = _facts(oracle, "triangle")
    assert (f["nn"], f["m"], f["max_deg"]) == (3, 3, 2) and CC.fx_bits_of(f["max_deg"]) == 60 and np.all(f["nact"] == 1) and np.all(f["cnt"] == 1)
    f = _facts(oracle, "K64")
    assert f["m"] == 64 * 63 // 2 and f["max_deg"] + 1 == 64 and CC.fx_bits_of(f["max_deg"]) == 56 and np.all(f["nact"] == 62)
    f = _facts(oracle, "er40")
    assert (f["cnt"].min(), f["cnt"].max()) == (3, 20) and abs(f["avg_run"] - 10.45) < 0.005 and f["avg_run"] <= 10.5
    assert np.count_nonzero(f["nact_seg"] > 16) == 6 and f["nact"].max() <= 32           # six segments take a second round at 8 lanes, none a third
    f = _facts(oracle, "er200")
    assert abs(f["avg_run"] - 8.07) < 0.005 and f["nact"].max() <= 20 and f["sampled"] < 1.0
    f = _facts(oracle, "er60_full")
    assert f["sampled"] == 1.0 and (f["nact"].min(), f["nact"].max()) == (39, 56)
    assert (CC.rounds(39, 16), CC.rounds(56, 16), CC.rounds(39, 8), CC.rounds(56, 8)) == (2, 2, 3, 4)
    f = _facts(oracle, "er150_full")
    assert f["nact"].max() == 97 and (CC.rounds(97, 16), CC.rounds(97, 8)) == (4, 7) and f["avg_run"] > 10.5
    f = _facts(oracle, "bridged150_60")
    assert f["m_pos"] < f["m"]                                      # edges without cycles ...
    st = CC.structure(oracle, "bridged150_60")
    nn, ii, jj, rij = CC.graph("bridged150_60")
    bare = np.setdiff1d(np.arange(f["m"]), st["pos_edge"][:f["m_pos"]])
    deg = np.bincount(np.concatenate([ii, jj]), minlength=nn)
    assert bare.size == 5 and bare.min() > 0 and bare.max() < f["m"] - 1                    # ... inside the edge list,
    assert np.all(deg[ii[bare]] > 1) and np.all(deg[jj[bare]] > 1)                          # in rows that hold segments with cycles too: zero-length runs
    for case in HOST_CASES:
        assert _facts(oracle, case)["max_deg"] < 511                # never eligible for the wave-per-node path (4 * COLSUM_SHORT <= max_deg + 1)


def test_structural_claims_of_the_large_cases(oracle):
    """hub1500_mid and K258: structure only (their weight states run on the GPU)."""
    f = _facts(oracle, "hub1500_mid")
    assert f["max_deg"] == 1499 and CC.fx_bits_of(1499) == 51 and f["max_deg"] >= 4 * CC.COLSUM_SHORT - 1
    nn, ii, jj, rij = CC.graph("hub1500_mid")
    deg = np.bincount(np.concatenate([ii, jj]), minlength=nn)
    assert np.count_nonzero(deg > CC.COLSUM_SHORT) == 1 and deg.max() > 1024 and f["avg_run"] <= 10.5
    f = _facts(oracle, "K258")
    assert f["m"] == 258 * 257 // 2 and f["max_deg"] == 257 and CC.fx_bits_of(257) == 53
    assert np.all(f["nact"] == CC.MAX_SEG_CYCLES) and np.all(f["cnt"] == CC.MAX_SEG_CYCLES)
    assert (CC.rounds(256, 16), CC.rounds(256, 8)) == (CC.MAX_SEG_CYCLES // 32, CC.MAX_SEG_CYCLES // 16)         # the last round of both instances

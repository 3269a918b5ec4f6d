"""CPU tests (no GPU) of the batched device structure builder's host side: the ABI surface, the plan rule
(desc_test_batch_plan: n_sample, m_pos, m_cycle from a histogram of codegrees) against the oracle's build_structure, and the
refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import make_problem

# the mixed batch of tests/test_gpu_batch.py: (n, p, model seed)
MIXED = [(12, 0.6, 9), (40, 0.5, 10), (90, 0.5, 8), (150, 0.95, 6), (200, 0.5, 4)]
NEW_SYMBOLS = ["desc_pgd_batch_create_where", "desc_pgd_batch_built_where", "desc_pgd_batch_max_codeg", "desc_pgd_batch_build_laps",
               "desc_test_batch_plan"]


def complete(n):
    ii, jj = np.triu_indices(n, 1)
    return n, ii.astype(np.int32), jj.astype(np.int32)


def cliques(sizes):
    """A disjoint union of complete graphs, Ind sorted by (i, j): every edge of a K_a has codegree a - 2."""
    ii, jj, base = [], [], 0
    for a in sizes:
        i, j = np.triu_indices(a, 1)
        ii.append(i + base); jj.append(j + base); base += a
    return base, np.concatenate(ii).astype(np.int32), np.concatenate(jj).astype(np.int32)


def plan_vs_oracle(lib, oracle, n, ii, jj, n_sample_min=30):
    st = oracle.build_structure(n, ii, jj, seed=1, n_sample_min=n_sample_min)
    hist = np.bincount(st["codeg"], minlength=n + 1)
    got = lib.batch_plan(hist, n_sample_min)
    assert (got["n_sample"], got["m_pos"], got["m_cycle"]) == (st["n_sample"], st["m_pos"], st["m_cycle"])
    cd = st["codeg"]
    assert got["max_codeg"] == (int(cd.max()) if cd.size else 0) and got["max_cnt"] == min(got["max_codeg"], got["n_sample"])
    return st, got


def test_new_symbols_exist(lib):
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS, name
    assert C.sizeof(lib.BatchResult) == 104          # the result record keeps its layout
    assert 64 <= lib.pgd_batch_max_codeg() <= lib.cemp_batch_max_degree()
    assert 4 * lib.pgd_batch_max_codeg() * 12 <= 64 * 1024          # key + packed positions per staged neighbour, 4 waves


@pytest.mark.parametrize("case", range(len(MIXED)))
def test_plan_rule_on_the_mixed_problems(lib, oracle, case):
    n, p, seed = MIXED[case]
    mo, nn, ii, jj, rij = make_problem("uniform", n=n, p=p, q=0.2, sigma=0.1, seed=seed)
    st, got = plan_vs_oracle(lib, oracle, nn, ii, jj)
    if case == 3:
        assert got["n_sample"] == 34
    # a floor that never binds: the median alone decides
    plan_vs_oracle(lib, oracle, nn, ii, jj, n_sample_min=1)


def test_plan_rule_on_an_empty_histogram(lib, oracle):
    """No edge has a cycle: median([]) = NaN and max(NaN, 30) = 30."""
    for n in (0, 1, 8):
        got = lib.batch_plan(np.zeros(n + 1, dtype=np.int32))
        assert got == dict(m_pos=0, max_codeg=0, n_sample=30, m_cycle=0, max_cnt=0)
    hist = np.zeros(9, dtype=np.int32); hist[0] = 7            # the path graph of tests/test_gpu_batch.py
    assert lib.batch_plan(hist, 12) == dict(m_pos=0, max_codeg=0, n_sample=12, m_cycle=0, max_cnt=0)
    ii = np.arange(7, dtype=np.int32)
    plan_vs_oracle(lib, oracle, 8, ii, ii + 1)


def test_plan_rule_median_of_an_even_count(lib, oracle):
    """11 x K6 and 3 x K11: 165 edges of codegree 4 and 165 of codegree 9.  MATLAB's median is 6.5, so ceil(6.5 / 4) = 2, where the
    lower middle value alone gives 1 and the upper one 3."""
    n, ii, jj = cliques([6] * 11 + [11] * 3)
    st, got = plan_vs_oracle(lib, oracle, n, ii, jj, n_sample_min=1)
    pos = np.sort(st["codeg"][st["codeg"] > 0])
    assert pos.size == 330 and (pos[164], pos[165]) == (4, 9)
    assert got["n_sample"] == 2 and got["m_cycle"] == 2 * 330
    plan_vs_oracle(lib, oracle, n, ii, jj)                      # and with the floor of 30


def test_plan_rule_median_of_an_odd_count(lib, oracle):
    """Uniform_Topology(16, 0.6, seed 19): 71 edges with cycles, the middle value 5 with a 4 below it."""
    mo, nn, ii, jj, rij = make_problem("uniform", n=16, p=0.6, seed=19)
    st, got = plan_vs_oracle(lib, oracle, nn, ii, jj, n_sample_min=1)
    pos = np.sort(st["codeg"][st["codeg"] > 0])
    assert pos.size == 71 and (pos[34], pos[35]) == (4, 5)
    assert got["n_sample"] == 2


@pytest.mark.parametrize("n, codeg, n_sample", [(31, 29, 30), (32, 30, 30), (33, 31, 30), (258, 256, 64), (259, 257, 65)])
def test_plan_rule_on_complete_graphs(lib, oracle, n, codeg, n_sample):
    """K31: no edge is sampled.  K32: every codegree equals n_sample, the sampling branch runs with nothing to drop.  K33: 30 of 31.
    K258: n_sample = 64, the largest a batch takes.  K259: 65, refused."""
    nn, ii, jj = complete(n)
    st, got = plan_vs_oracle(lib, oracle, nn, ii, jj)
    assert set(st["codeg"].tolist()) == {codeg}
    assert got["n_sample"] == n_sample and got["m_pos"] == n * (n - 1) // 2 and got["m_cycle"] == got["m_pos"] * min(codeg, n_sample)


def test_build_argument_is_checked_before_any_library_call(lib, monkeypatch):
    from desc_amd import ConstantStepSize, DESC_batch, DESC_init_batch, DESC_PGD_batch
    mo, *_ = make_problem("uniform", n=20, p=0.5, seed=1)

    def no_library(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(lib, "Batch", no_library)
    monkeypatch.setattr(lib, "load", no_library)
    ok = dict(iters=3, Gradient=ConstantStepSize(0.01), verbose=False)
    for call in (DESC_PGD_batch, DESC_init_batch, DESC_batch):
        for bad in ("hose", "", None, 1, "Device"):
            with pytest.raises(ValueError, match="build"):
                call([mo], ok, build=bad)


def test_create_where_refuses_an_unknown_builder(lib):
    mo, nn, ii, jj, rij = make_problem("uniform", n=20, p=0.5, seed=1)
    prob = lib.ProblemArrays(nn, ii, jj, rij)
    h = C.c_void_p(1)
    p = lib.default_params()
    rc = lib.load().desc_pgd_batch_create_where(C.byref(prob.c), 1, C.byref(p), None, 7, C.byref(h))
    assert rc == lib.ERR_INVALID and not h.value
    assert b"where = 7" in lib.load().desc_last_error()
    with pytest.raises(lib.DescError) as ei:
        lib.Batch([prob], p, None, 7)
    assert ei.value.code == lib.ERR_INVALID

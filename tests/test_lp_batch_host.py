"""CPU tests (no GPU) of the batched LP's host side (desc_lp_batch_*, _lib.LpBatch, linprog_sij_batch): ABI surface, the struct sizes the
header states, the refusals that come before any device call and name the problem, the per-problem nsample rule, offsets and virtual
grids of desc_lp_batch_plan (the host half of create) against tests/lp_oracle.py, the empty batch, a NULL handle."""
import ctypes as C

import numpy as np
import pytest

from desc_amd.algorithms import _marshal_problems
from tests import graph_shapes as gs
from tests import lp_cases as LC

SYMBOLS = ["desc_lp_batch_plan", "desc_lp_batch_create", "desc_lp_batch_sizes", "desc_lp_batch_get_samples", "desc_lp_batch_run",
           "desc_lp_batch_destroy"]


def test_abi_surface(lib):
    import desc_amd
    L = lib.load()
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/desc_amd.h").read()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS and name + "(" in hdr, name
    assert C.sizeof(lib.LpBatchTimings) == 40      # as include/desc_amd.h states: 5 doubles
    assert "} desc_lp_batch_timings;      /* 40 bytes */" in hdr
    assert [f for f, _ in lib.LpBatchTimings._fields_] == ["ms_structure", "ms_upload", "ms_build", "ms_loop", "ms_total"]
    assert C.sizeof(lib.LpParams) == 48 and "} desc_lp_params;             /* 48 bytes */" in hdr
    assert C.sizeof(lib.LpInfo) == 104 and "} desc_lp_info;               /* 104 bytes */" in hdr
    assert callable(desc_amd.linprog_sij_batch) and "linprog_sij_batch" in desc_amd.__all__
    for name in ("run", "samples", "sizes", "destroy"):
        assert callable(getattr(lib.LpBatch, name))


def test_refusals_come_before_any_device_call(lib, monkeypatch):
    from desc_amd import linprog_sij_batch

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    for name in ("LpBatch", "GcwBatch", "RefineBatch"):
        monkeypatch.setattr(lib, name, no_device)
    mo = LC.model("n30")
    for rotations in (True, False):
        kw = dict(rotations=rotations)
        for bad in (mo, 7, None, np.zeros(3), "ab"):
            with pytest.raises(ValueError, match="sequence"):
                linprog_sij_batch(bad, **kw)
        with pytest.raises(ValueError, match="problem 1: empty edge list"):
            linprog_sij_batch([mo, (np.zeros((0, 2)), np.zeros((3, 3, 0)))], **kw)
        with pytest.raises(ValueError, match="problem 1: expected an"):
            linprog_sij_batch([mo, 5], **kw)
        with pytest.raises(ValueError, match=r"problem 1: nsample = -2, need nsample >= 0"):
            linprog_sij_batch([mo, mo], dict(nsample=[0, -2]), **kw)
        with pytest.raises(ValueError, match=r"problem 0: nsample = -1"):
            linprog_sij_batch([mo, mo], dict(nsample=-1), **kw)
        with pytest.raises(ValueError, match=r"nsample must hold one entry per problem \(2\), not 3"):
            linprog_sij_batch([mo, mo], dict(nsample=[7, 7, 7]), **kw)
        with pytest.raises(ValueError, match=r"seeds must hold one entry per problem \(2\), not 1"):
            linprog_sij_batch([mo, mo], seeds=[1], **kw)
        cap = lib.cemp_batch_max_degree()
        assert cap == 4096
        with pytest.raises(ValueError, match=f"problem 1: node 0 has {cap + 1} neighbours, more than the {cap} the batched sampler stages") as ei:
            linprog_sij_batch([mo, gs.star(cap + 2, 1, seed=3)], **kw)
        assert "solve it with linprog_sij" in str(ei.value)
        assert linprog_sij_batch([], **kw) == [] and linprog_sij_batch([], return_info=True, **kw) == []
    # the eigen-solve's cap holds only where rotations are asked for
    ncap = lib.gcw_batch_max_n()
    assert ncap == 278
    big = gs.band(ncap + 1, 2, seed=2)
    with pytest.raises(ValueError, match=f"problem 1: n = {ncap + 1} exceeds {ncap}") as ei:
        linprog_sij_batch([mo, big])
    assert "solve it with linprog_sij" in str(ei.value) and "rotations=False" in str(ei.value)
    with pytest.raises(AssertionError, match="asked for a device"):      # nothing on the host refuses it: the call goes on to the device
        linprog_sij_batch([mo, big], rotations=False)


def test_rows_beyond_the_index_budget_are_refused_on_the_host(lib):
    """2 * sum(m_pos_b * nsample_b) >= 2^31: band(n, 2) has 2 n - 3 variables, so 3 problems of 2001 variables with 180000 samples each."""
    from desc_amd import linprog_sij_batch
    mo = gs.band(1002, 2, seed=9)
    probs, _ = _marshal_problems([mo] * 3)
    ns = 180000
    assert 2 * 2 * 2001 * ns < 2 ** 31 <= 3 * 2 * 2001 * ns
    lib.lp_batch_plan(probs[:2], ns)
    with pytest.raises(lib.DescError, match="problems 0 to 2 hold .* split the batch") as ei:
        lib.lp_batch_plan(probs, ns)
    assert ei.value.code == lib.ERR_TOO_LARGE
    with pytest.raises(ValueError, match="split the batch"):
        linprog_sij_batch([mo] * 3, dict(nsample=ns), rotations=False)


@pytest.mark.parametrize("graph", ["n30", "sparse", "hub60", "star12"])
def test_plan_follows_the_rule_per_problem(lib, graph):
    """nsample by the rule of linprog_sij.m:43, m_pos, the offsets and the virtual grids (grid_for of lp.hip) of a problem inside a batch."""
    probs, _ = _marshal_problems([LC.model("book33"), LC.model(graph), LC.model("n30_s5")])
    own, va, vb, d, pos, k, ns = LC.arrays(graph)
    pl = lib.lp_batch_plan(probs, [32, None, 33])
    assert pl["nsample"].tolist() == [32, ns, 33]
    assert pl["m_pos"][1] == pos.size and pl["m_pos"][0] == LC.arrays("book33", 32)[4].size
    assert np.array_equal(np.diff(pl["var_off"]), pl["m_pos"]) and np.array_equal(np.diff(pl["row_off"]), pl["m_pos"] * pl["nsample"])
    for b in range(3):
        mp, nsb = int(pl["m_pos"][b]), int(pl["nsample"][b])
        per = 8 if nsb <= 32 else 4
        assert pl["ncol"][b] == (min(2048, -(-mp // 16)) if mp else 0) and pl["nrow"][b] == (min(4096, -(-mp // per)) if mp else 0)
    alone = lib.lp_batch_plan(probs[1:2])
    assert alone["nsample"][0] == ns and alone["m_pos"][0] == pos.size


def test_rule_above_its_floor_and_grids_at_their_caps(lib):
    """K_130: every codegree is 128, the rule gives ceil(128 / 4) = 32 > 30.  U370 with 8 and U270 with 40 samples: the virtual grids at
    their caps of 2048 and 4096 blocks."""
    from tests import lp_oracle as O
    n = 130
    iu = np.triu_indices(n, 1)
    Ind = np.stack([iu[0] + 1, iu[1] + 1], axis=1)
    Rij = np.repeat(np.eye(3)[:, :, None], Ind.shape[0], axis=2)
    probs, _ = _marshal_problems([(Ind, Rij), LC.model("U370"), LC.model("U270")])
    assert O.rule_nsample(np.full(Ind.shape[0], n - 2)) == 32
    pl = lib.lp_batch_plan(probs, [None, 8, 40])
    assert pl["nsample"].tolist() == [32, 8, 40] and pl["m_pos"][0] == Ind.shape[0]
    assert pl["m_pos"][1] > 32768 and pl["ncol"][1] == 2048 and pl["nrow"][1] == 4096
    assert pl["m_pos"][2] > 16384 and pl["nrow"][2] == 4096 and pl["ncol"][2] == -(-int(pl["m_pos"][2]) // 16)


def test_c_entry_points_refuse_a_null_handle(lib):
    L = lib.load()
    assert L.desc_lp_batch_run(None, None, None, None, None, None) == lib.ERR_INVALID
    assert b"NULL handle" in L.desc_last_error()
    assert L.desc_lp_batch_sizes(None, None, None, None, None, None, None, None) == lib.ERR_INVALID
    assert L.desc_lp_batch_get_samples(None, None, None) == lib.ERR_INVALID
    L.desc_lp_batch_destroy(None)
    h = C.c_void_p(5)
    assert L.desc_lp_batch_create(None, 2, None, None, 0, C.byref(h)) == lib.ERR_INVALID and not h.value


def test_empty_handle_runs_and_returns_nothing(lib):
    b = lib.LpBatch([])
    assert b.count == 0 and b.sizes() == [] and b.samples() == []
    outs, timings = b.run()
    assert outs == [] and timings["ms_loop"] == 0
    outs, _ = b.run(lib.default_lp_params(), want_y=True)
    assert outs == []
    p = lib.default_lp_params()
    p.max_iter = -1
    with pytest.raises(lib.DescError, match="need max_iter >= 0") as ei:
        b.run(p)
    assert ei.value.code == lib.ERR_INVALID
    b.destroy()
    assert lib.lp_batch_plan([])["var_off"].tolist() == [0]

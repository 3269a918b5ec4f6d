"""CPU tests (no GPU) of the batched CEMP baselines' host side (desc_cemp_batch_*, desc_mst_batch_*, CEMP_batch, CEMP_GCW_batch,
MST_batch, CEMP_MST_batch): ABI surface, caps, refusals that come before any device call, create without a device, the empty batch."""
import ctypes as C

import numpy as np
import pytest

from desc_amd.algorithms import marshal_edges
from tests import cemp_batch_cases as cases
from tests import graph_shapes as gs

SYMBOLS = ["desc_cemp_batch_max_degree", "desc_cemp_batch_create", "desc_cemp_batch_sizes", "desc_cemp_batch_get_samples", "desc_cemp_batch_run",
           "desc_cemp_batch_destroy", "desc_mst_batch_max_n", "desc_mst_batch_check", "desc_mst_batch_run"]


def _arrays(lib, mo):
    n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None
    return lib.ProblemArrays(n, ii, jj, rij)


def test_abi_surface(lib):
    import desc_amd
    L = lib.load()
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/desc_amd.h").read()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS and name + "(" in hdr, name
    assert C.sizeof(lib.CempBatchTimings) == 40 and C.sizeof(lib.MstBatchTimings) == 40      # as include/desc_amd.h states: 5 doubles each
    for name in ("CEMP_batch", "CEMP_GCW_batch", "MST_batch", "CEMP_MST_batch"):
        assert callable(getattr(desc_amd, name)) and name in desc_amd.__all__
    assert lib.cemp_batch_max_degree() >= 512 and lib.mst_batch_max_n() >= 1024
    # the sampler packs two row positions in 16 bits each; 4 waves x cap positions x 4 B and 16 B per node fit the 64 KiB every launch may declare
    assert lib.cemp_batch_max_degree() <= 65536 and 16 * lib.cemp_batch_max_degree() <= 64 * 1024 and 16 * lib.mst_batch_max_n() <= 64 * 1024


def test_refusals_come_before_any_device_call(lib, monkeypatch):
    from desc_amd import CEMP_GCW_batch, CEMP_MST_batch, CEMP_batch, MST_batch
    mo = cases.model("U12")
    m = mo.Ind.shape[0]
    S = gs.noisy_truth(mo, 1)
    ok = cases.params()

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    for name in ("CempBatch", "GcwBatch", "mst_batch_run"):
        monkeypatch.setattr(lib, name, no_device)
    calls = (CEMP_batch, CEMP_GCW_batch, CEMP_MST_batch)
    for call in calls:
        for bad in (mo, 7, None, np.zeros(3), "ab"):
            with pytest.raises(ValueError, match="sequence"):
                call(bad, ok)
        empty = (np.zeros((0, 2)), np.zeros((3, 3, 0)))
        with pytest.raises(ValueError, match="problem 1: empty edge list"):
            call([mo, empty], ok)
        with pytest.raises(ValueError, match="seeds must hold one entry per problem \\(2\\), not 1"):
            call([mo, mo], ok, seeds=[1])
        with pytest.raises(ValueError, match="nsample"):
            call([mo], dict(ok, nsample=0))
        with pytest.raises(ValueError, match="max_iter"):
            call([mo], dict(ok, max_iter=-1))
        with pytest.raises(ValueError, match="reweighting"):
            call([mo], dict(ok, reweighting=[]))
        with pytest.raises(ValueError, match="reweighting"):
            call([mo], {k: v for k, v in ok.items() if k != "reweighting"})
        assert call([], ok) == []
    # a node above the sampler's staging cap
    cap = lib.cemp_batch_max_degree()
    star = gs.star(cap + 2, 1, seed=3)
    for call in calls:
        with pytest.raises(ValueError, match=f"problem 1: node 0 has {cap + 1} neighbours") as ei:
            call([mo, star], ok)
        assert "solve it with CEMP" in str(ei.value)
    # the eigen-solve's size cap
    gcap = lib.gcw_batch_max_n()
    with pytest.raises(ValueError, match=f"problem 1: n = {gcap + 1} exceeds {gcap}"):
        CEMP_GCW_batch([mo, gs.band(gcap + 1, 1, seed=2)], ok)
    # the tree kernel's: size cap, S_list, connectivity
    tcap = lib.mst_batch_max_n()
    big = gs.band(tcap + 1, 1, seed=2)
    with pytest.raises(ValueError, match=f"problem 1: n = {tcap + 1} exceeds {tcap}") as ei:
        MST_batch([mo, big], [S, np.zeros(tcap)])
    assert "solve it with MST" in str(ei.value)
    with pytest.raises(ValueError, match=f"problem 1: n = {tcap + 1} exceeds {tcap}"):
        CEMP_MST_batch([mo, big], ok)
    for bad in (mo, 7, None, np.zeros(3), "ab"):
        with pytest.raises(ValueError, match="sequence"):
            MST_batch(bad, [S])
    with pytest.raises(ValueError, match="one SVec per problem"):
        MST_batch([mo, mo], [S])
    with pytest.raises(ValueError, match="one SVec per problem"):
        MST_batch([mo], S)
    with pytest.raises(ValueError, match=f"problem 1: SVec must have one entry per edge \\({m}\\), not {m - 1}"):
        MST_batch([mo, mo], [S, S[:-1]])
    for bad in (np.nan, np.inf, -np.inf):
        Sb = S.copy(); Sb[5] = bad
        with pytest.raises(ValueError, match="problem 1: SVec entry 5 is not finite"):
            MST_batch([mo, mo], [S, Sb])
    with pytest.raises(ValueError, match="problem 0: empty edge list"):
        MST_batch([(np.zeros((0, 2)), np.zeros((3, 3, 0)))], [np.zeros(0)])
    Ind2, R2 = cases.two_triangles()
    with pytest.raises(ValueError, match="problem 1: the graph is disconnected: 2 components"):
        MST_batch([mo, (Ind2, R2)], [S, np.zeros(6)])
    with pytest.raises(ValueError, match="problem 0: the graph is disconnected: 2 components"):
        CEMP_MST_batch([(Ind2, R2), mo], ok)
    Ind_gap = np.array([[1, 2], [1, 3], [2, 3], [3, 5]])                                  # node 4 touches no edge
    with pytest.raises(ValueError, match="problem 0: the graph is disconnected: 2 components"):
        MST_batch([(Ind_gap, R2[:, :, :4])], [np.zeros(4)])
    assert MST_batch([], []) == []


def test_c_entry_points_refuse_before_the_device(lib):
    """The C entry points: DESC_ERR_INVALID naming the problem -- the same message with and without a GPU -- and *out stays NULL."""
    L = lib.load()
    mo = cases.model("U12")
    cap = lib.cemp_batch_max_degree()
    probs = [_arrays(lib, mo), _arrays(lib, gs.star(cap + 2, 1, seed=3))]
    with pytest.raises(lib.DescError) as ei:
        lib.CempBatch(probs, 10)
    assert ei.value.code == lib.ERR_INVALID
    assert f"problem 1: node 0 has {cap + 1} neighbours" in str(ei.value) and "solve it with CEMP" in str(ei.value)
    arr = (lib.Problem * 2)(*[q.c for q in probs])
    h = C.c_void_p(1)
    assert L.desc_cemp_batch_create(arr, 2, 10, 0, None, 0, C.byref(h)) == lib.ERR_INVALID and not h.value
    h = C.c_void_p(1)
    assert L.desc_cemp_batch_create(arr, 1, 0, 0, None, 0, C.byref(h)) == lib.ERR_INVALID and not h.value       # nsample < 1
    empty = lib.ProblemArrays(3, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    with pytest.raises(lib.DescError, match="problem 1: empty edge list"):
        lib.CempBatch([probs[0], empty], 10)
    # m_total * nsample >= 2^31
    with pytest.raises(lib.DescError) as ei:
        lib.CempBatch([probs[0]], 2 ** 31 // probs[0].m + 1)
    assert ei.value.code == lib.ERR_TOO_LARGE
    # the tree step: check and run give the same refusals, run before it looks for a device
    Ind2, R2 = cases.two_triangles()
    n, ii, jj, rij, _ = marshal_edges(Ind2, R2)
    tri = lib.ProblemArrays(n, ii, jj, rij)
    lib.mst_batch_check([probs[0]])
    for call in (lambda: lib.mst_batch_check([probs[0], tri]), lambda: lib.mst_batch_run([probs[0], tri], np.zeros(probs[0].m + 6))):
        with pytest.raises(lib.DescError, match="problem 1: the graph is disconnected: 2 components") as ei:
            call()
        assert ei.value.code == lib.ERR_INVALID
    Sb = np.zeros(probs[0].m); Sb[7] = np.nan
    with pytest.raises(lib.DescError, match="problem 0: S_vec entry 7 is not finite"):
        lib.mst_batch_run([probs[0]], Sb)


def test_create_without_a_device_fails_with_err_hip(lib):
    if lib.load().desc_device_count() > 0:
        pytest.skip("a GPU is visible")
    prob = _arrays(lib, cases.model("U12"))
    with pytest.raises(lib.DescError) as ei:
        lib.CempBatch([prob, prob], 10)
    assert ei.value.code == lib.ERR_HIP
    h = C.c_void_p(1)
    rc = lib.load().desc_cemp_batch_create(C.byref(prob.c), 1, 10, 0, None, 0, C.byref(h))
    assert rc == lib.ERR_HIP and not h.value and lib.load().desc_last_error()
    with pytest.raises(lib.DescError) as ei:
        lib.mst_batch_run([prob], np.zeros(prob.m))
    assert ei.value.code == lib.ERR_HIP


def test_empty_batch_through_the_c_abi(lib):
    b = lib.CempBatch([], 10)
    assert b.count == 0 and b.n == 0 and b.m == 0
    outs, timings = b.run([1.0], 3)
    assert outs == [] and timings["ms_rounds"] == 0
    assert b.samples() == []
    b.destroy()
    outs, timings = lib.mst_batch_run([], np.zeros(0))
    assert outs == [] and timings["ms_tree"] == 0

"""CPU tests (no GPU) of the batched refinement's host side (desc_refine_batch_*, DESC_refine_batch, DESC_batch): ABI surface, the size
cap, refusals that come before any device call and name the problem, the empty batch, create without a device."""
import ctypes as C

import numpy as np
import pytest

from desc_amd import ConstantStepSize
from desc_amd.algorithms import marshal_edges
from tests import graph_shapes as gs
from tests.helpers import make_problem

REFINE_BATCH_SYMBOLS = ["desc_refine_batch_max_n", "desc_refine_batch_create", "desc_refine_batch_sizes", "desc_refine_batch_run",
                        "desc_refine_batch_destroy"]


def _arrays(lib, mo):
    n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None
    return lib.ProblemArrays(n, ii, jj, rij)


def _eye(n):
    return np.asfortranarray(np.repeat(np.eye(3)[:, :, None], n, axis=2))


def test_refine_batch_abi_surface(lib):
    import desc_amd
    L = lib.load()
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/desc_amd.h").read()
    for name in REFINE_BATCH_SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS and name + "(" in hdr, name
    assert C.sizeof(lib.RefineBatchTimings) == 40    # as include/desc_amd.h states: 5 doubles
    assert "} desc_refine_batch_timings;  /* 40 bytes */" in hdr
    assert C.sizeof(lib.RefineInfo) == 40
    for name in ("DESC_batch", "DESC_refine_batch"):
        assert callable(getattr(desc_amd, name)) and name in desc_amd.__all__


def test_size_cap_covers_the_eigen_solve(lib):
    cap = lib.refine_batch_max_n()
    assert cap >= 278 and cap >= lib.gcw_batch_max_n()


def test_refusals_come_before_any_device_call(lib, monkeypatch):
    from desc_amd import DESC_batch, DESC_refine_batch
    mo, *_ = make_problem("uniform", n=20, p=0.5, seed=1)
    cap, gcap = lib.refine_batch_max_n(), lib.gcw_batch_max_n()
    big, gbig = gs.band(cap + 1, 1, seed=2), gs.band(gcap + 1, 1, seed=2)
    S, Sbig = gs.noisy_truth(mo, 1), gs.noisy_truth(big, 2)
    R0, Rbig = _eye(20), _eye(cap + 1)

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    for name in ("Batch", "GcwBatch", "RefineBatch"):
        monkeypatch.setattr(lib, name, no_device)
    ok = dict(iters=3, Gradient=ConstantStepSize(0.01), verbose=False)
    with pytest.raises(ValueError, match=f"problem 1: n = {cap + 1} exceeds {cap}") as ei:
        DESC_refine_batch([mo, big], [S, Sbig], [R0, Rbig])
    assert "solve it with DESC" in str(ei.value)
    with pytest.raises(ValueError, match="one S_vec per problem"):
        DESC_refine_batch([mo, mo], [S], [R0, R0])
    with pytest.raises(ValueError, match="one R_init per problem"):
        DESC_refine_batch([mo, mo], [S, S], [R0])
    with pytest.raises(ValueError, match="one R_init per problem"):
        DESC_refine_batch([mo], [S], 7)
    with pytest.raises(ValueError, match="problem 1: S_vec must have one entry per edge"):
        DESC_refine_batch([mo, mo], [S, S[:-1]], [R0, R0])
    with pytest.raises(ValueError, match="problem 1: R_init must be 3 x 3 x 20, not 3 x 3 x 19"):
        DESC_refine_batch([mo, mo], [S, S], [R0, R0[:, :, :-1]])
    for bad in (-1e-3, np.nan, np.inf):
        Sb = S.copy(); Sb[5] = bad
        with pytest.raises(ValueError, match=f"problem 1: S_vec holds a negative or non-finite entry \\(node {int(mo.Ind[5, 0]) - 1}\\)"):
            DESC_refine_batch([mo, mo], [S, Sb], [R0, R0])
    for bad in (np.nan, -np.inf):
        Rb = R0.copy(); Rb[1, 2, 4] = bad
        with pytest.raises(ValueError, match="problem 0: R_init holds a non-finite entry \\(node 4\\)"):
            DESC_refine_batch([mo, mo], [S, S], [Rb, R0])
    empty = (np.zeros((0, 2)), np.zeros((3, 3, 0)))
    with pytest.raises(ValueError, match="problem 1: empty edge list"):
        DESC_refine_batch([mo, empty], [S, np.zeros(0)], [R0, np.zeros((3, 3, 0))])
    for bad in (mo, 7, None, np.zeros(3), "ab"):
        with pytest.raises(ValueError, match="sequence"):
            DESC_refine_batch(bad, [S], [R0])
        with pytest.raises(ValueError, match="sequence"):
            DESC_batch(bad, ok)
    # DESC_batch refuses what DESC_init_batch refuses, in its words
    from desc_amd import DESC_init_batch

    class Plug:
        calls = 0

        def GetStep(self, g):
            self.calls += 1
            return -0.01 * g
    plug = Plug()
    for args, kw in ((([mo, gbig], ok), {}), (([mo, empty], ok), {}), (([mo], dict(ok, Gradient=plug)), {}),
                     (([mo], dict(ok, make_plots=True, ErrVec=mo.ErrVec, R_orig=mo.R_orig)), {}), (([mo, mo], ok), dict(seeds=[1]))):
        with pytest.raises(ValueError) as e_init:
            DESC_init_batch(*args, **kw)
        with pytest.raises(ValueError) as e_batch:
            DESC_batch(*args, **kw)
        assert str(e_batch.value) == str(e_init.value)
    assert plug.calls == 0
    assert DESC_refine_batch([], [], []) == [] and DESC_batch([], ok) == []


def test_create_and_run_refuse_before_the_device(lib):
    """The C entry points: DESC_ERR_INVALID naming the problem -- the same message with and without a GPU -- and *out stays NULL."""
    mo, *_ = make_problem("uniform", n=20, p=0.5, seed=1)
    cap = lib.refine_batch_max_n()
    probs = [_arrays(lib, mo), _arrays(lib, gs.band(cap + 1, 1, seed=2))]
    with pytest.raises(lib.DescError) as ei:
        lib.RefineBatch(probs)
    assert ei.value.code == lib.ERR_INVALID
    assert f"problem 1: n = {cap + 1} exceeds {cap}" in str(ei.value) and "solve it with DESC" in str(ei.value)
    arr = (lib.Problem * 2)(*[q.c for q in probs])
    h = C.c_void_p(1)
    assert lib.load().desc_refine_batch_create(arr, 2, 0, C.byref(h)) == lib.ERR_INVALID and not h.value
    empty = lib.ProblemArrays(3, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    with pytest.raises(lib.DescError, match="problem 1: empty edge list"):
        lib.RefineBatch([probs[0], empty])
    unsorted = lib.ProblemArrays(3, np.array([1, 0], np.int32), np.array([2, 1], np.int32), np.tile(np.eye(3).reshape(-1), 2))
    with pytest.raises(lib.DescError, match="problem 1: ") as ei:
        lib.RefineBatch([probs[0], unsorted])
    assert ei.value.code == lib.ERR_INVALID
    assert lib.load().desc_refine_batch_create(None, 1, 0, C.byref(h)) == lib.ERR_INVALID
    assert lib.load().desc_refine_batch_create(arr, -1, 0, C.byref(h)) == lib.ERR_INVALID
    assert lib.load().desc_refine_batch_run(None, None, None, 0.0, 0, None, None, None) == lib.ERR_INVALID


def test_create_without_a_device_fails_with_err_hip(lib):
    if lib.load().desc_device_count() > 0:
        pytest.skip("a GPU is visible")
    mo, *_ = make_problem("uniform", n=20, p=0.5, seed=1)
    prob = _arrays(lib, mo)
    with pytest.raises(lib.DescError) as ei:
        lib.RefineBatch([prob, prob])
    assert ei.value.code == lib.ERR_HIP
    h = C.c_void_p(1)
    rc = lib.load().desc_refine_batch_create(C.byref(prob.c), 1, 0, C.byref(h))
    assert rc == lib.ERR_HIP and not h.value and lib.load().desc_last_error()


def test_empty_batch_through_the_c_abi(lib):
    b = lib.RefineBatch([])
    assert b.count == 0 and b.n == 0 and b.m == 0
    outs, timings = b.run(np.zeros(0), np.zeros(0))
    assert outs == [] and timings["ms_refine"] == 0 and timings["ms_input"] == 0
    outs, _ = b.run(np.zeros(0), np.zeros(0), max_iters=2)     # a handle can be run again
    assert outs == []
    b.destroy()

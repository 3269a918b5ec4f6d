"""CPU tests (no GPU) of the batched Spectral / GCW eigen-solve's host side (desc_gcw_batch_*, Spectral_batch, GCW_batch,
DESC_init_batch): ABI surface, the size cap, refusals that come before any device call, the per-problem CSR against NumPy."""
import ctypes as C

import numpy as np
import pytest

from desc_amd import ConstantStepSize
from desc_amd.algorithms import marshal_edges
from tests import graph_shapes as gs
from tests import gcw_batch_cases as cases
from tests.helpers import make_problem

GCW_BATCH_SYMBOLS = ["desc_gcw_batch_max_n", "desc_gcw_batch_create", "desc_gcw_batch_sizes", "desc_gcw_batch_csr", "desc_gcw_batch_run",
                     "desc_gcw_batch_destroy"]


class _Counting:
    """A plugin of the caller's own: DESC_init_batch must refuse it without calling it."""
    calls = 0

    def GetStep(self, g):
        self.calls += 1
        return -0.01 * g


def _arrays(lib, mo):
    n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None
    return lib.ProblemArrays(n, ii, jj, rij)


def test_gcw_batch_abi_surface(lib):
    L = lib.load()
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/desc_amd.h").read()
    for name in GCW_BATCH_SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS and name + "(" in hdr, name
    assert C.sizeof(lib.GcwBatchTimings) == 40       # as include/desc_amd.h states: 5 doubles
    assert C.sizeof(lib.SpectralInfo) == 56
    for name in ("Spectral_batch", "GCW_batch", "DESC_init_batch"):
        import desc_amd
        assert callable(getattr(desc_amd, name)) and name in desc_amd.__all__


def test_size_cap_covers_the_monte_carlo_sizes(lib):
    cap = lib.gcw_batch_max_n()
    assert cap >= 200
    # four 3n x 6 blocks of doubles and 448 doubles of small matrices within the 160 KiB a workgroup may declare; one more node does not fit
    assert (72 * cap + 448) * 8 <= 160 * 1024 < (72 * (cap + 1) + 448) * 8


def test_refusals_come_before_any_device_call(lib, monkeypatch):
    from desc_amd import DESC_init_batch, GCW_batch, Spectral_batch
    mo, *_ = make_problem("uniform", n=20, p=0.5, seed=1)
    cap = lib.gcw_batch_max_n()
    big = gs.band(cap + 1, 1, seed=2)
    S, Sbig = gs.noisy_truth(mo, 1), gs.noisy_truth(big, 2)

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(lib, "Batch", no_device)
    monkeypatch.setattr(lib, "GcwBatch", no_device)
    ok = dict(iters=3, Gradient=ConstantStepSize(0.01), verbose=False)
    over = f"problem 1: n = {cap + 1} exceeds {cap}"
    with pytest.raises(ValueError, match=over) as ei:
        Spectral_batch([mo, big])
    assert "GCW / DESC_init" in str(ei.value)
    with pytest.raises(ValueError, match=over):
        GCW_batch([mo, big], [S, Sbig])
    with pytest.raises(ValueError, match=over):
        DESC_init_batch([mo, big], ok)
    with pytest.raises(ValueError, match="one S_vec per problem"):
        GCW_batch([mo, mo], [S])
    with pytest.raises(ValueError, match="one S_vec per problem"):
        GCW_batch([mo], S)
    with pytest.raises(ValueError, match="problem 1: S_vec must have one entry per edge"):
        GCW_batch([mo, mo], [S, S[:-1]])
    for bad in (-1e-3, np.nan, np.inf):
        Sb = S.copy(); Sb[5] = bad
        with pytest.raises(ValueError, match=f"problem 1: S_vec holds a negative or non-finite entry \\(node {int(mo.Ind[5, 0]) - 1}\\)"):
            GCW_batch([mo, mo], [S, Sb])
    empty = (np.zeros((0, 2)), np.zeros((3, 3, 0)))
    with pytest.raises(ValueError, match="problem 1: empty edge list"):
        Spectral_batch([mo, empty])
    with pytest.raises(ValueError, match="problem 0: empty edge list"):
        GCW_batch([empty], [np.zeros(0)])
    with pytest.raises(ValueError, match="problem 1: empty edge list"):
        DESC_init_batch([mo, empty], ok)
    plug = _Counting()
    with pytest.raises(ValueError, match="GetStep"):
        DESC_init_batch([mo], dict(ok, Gradient=plug))
    assert plug.calls == 0
    with pytest.raises(ValueError, match="make_plots"):
        DESC_init_batch([mo], dict(ok, make_plots=True, ErrVec=mo.ErrVec, R_orig=mo.R_orig))
    with pytest.raises(ValueError, match="seeds"):
        DESC_init_batch([mo, mo], ok, seeds=[1])
    for bad in (mo, 7, None, np.zeros(3), "ab"):
        with pytest.raises(ValueError, match="sequence"):
            Spectral_batch(bad)
        with pytest.raises(ValueError, match="sequence"):
            DESC_init_batch(bad, ok)
    assert Spectral_batch([]) == [] and GCW_batch([], []) == [] and DESC_init_batch([], ok) == []


def test_create_refuses_an_oversized_problem_before_the_device(lib):
    """The C entry point: DESC_ERR_INVALID naming the problem -- the same message with and without a GPU -- and *out stays NULL."""
    mo, *_ = make_problem("uniform", n=20, p=0.5, seed=1)
    cap = lib.gcw_batch_max_n()
    probs = [_arrays(lib, mo), _arrays(lib, gs.band(cap + 1, 1, seed=2))]
    with pytest.raises(lib.DescError) as ei:
        lib.GcwBatch(probs)
    assert ei.value.code == lib.ERR_INVALID
    assert f"problem 1: n = {cap + 1} exceeds {cap}" in str(ei.value) and "GCW / DESC_init" in str(ei.value)
    arr = (lib.Problem * 2)(*[q.c for q in probs])
    h = C.c_void_p(1)
    assert lib.load().desc_gcw_batch_create(arr, 2, 0, C.byref(h)) == lib.ERR_INVALID and not h.value
    empty = lib.ProblemArrays(3, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    with pytest.raises(lib.DescError, match="problem 1: empty edge list"):
        lib.GcwBatch([probs[0], empty])


def test_create_without_a_device_fails_with_err_hip(lib):
    if lib.load().desc_device_count() > 0:
        pytest.skip("a GPU is visible")
    mo, *_ = make_problem("uniform", n=20, p=0.5, seed=1)
    prob = _arrays(lib, mo)
    with pytest.raises(lib.DescError) as ei:
        lib.GcwBatch([prob, prob])
    assert ei.value.code == lib.ERR_HIP
    h = C.c_void_p(1)
    rc = lib.load().desc_gcw_batch_create(C.byref(prob.c), 1, 0, C.byref(h))
    assert rc == lib.ERR_HIP and not h.value and lib.load().desc_last_error()


def test_empty_batch_through_the_c_abi(lib):
    b = lib.GcwBatch([])
    assert b.count == 0 and b.n == 0 and b.m == 0
    outs, timings = b.run(s_vec=np.zeros(0))
    assert outs == [] and timings["ms_eig"] == 0
    b.destroy()


def test_per_problem_csr_equals_numpy(lib):
    """desc_gcw_batch_csr on the mixed batch of the GPU tests: offsets, and every problem's CSR with LOCAL node and edge ids."""
    mos = cases.mixed_models(lib.gcw_batch_max_n())
    probs = [_arrays(lib, mo) for mo in mos]
    got = lib.gcw_batch_csr(probs)
    no = np.concatenate([[0], np.cumsum([q.n for q in probs])])
    eo = np.concatenate([[0], np.cumsum([q.m for q in probs])])
    assert np.array_equal(got["node_off"], no) and np.array_equal(got["edge_off"], eo)
    for b, q in enumerate(probs):
        rowptr, adj, eid = cases.csr_numpy(q.n, q.ind_i, q.ind_j)
        assert np.array_equal(got["rowptr"][no[b] + b:no[b + 1] + b + 1], rowptr), b
        assert np.array_equal(got["adj"][2 * eo[b]:2 * eo[b + 1]], adj), b
        assert np.array_equal(got["adj_eid"][2 * eo[b]:2 * eo[b + 1]], eid), b

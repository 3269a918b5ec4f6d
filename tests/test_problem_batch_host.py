"""CPU tests (no GPU) of the resident problem set's host side (desc_problem_batch_*, the *_create_on calls, ProblemBatch): ABI surface,
the empty set, NULL arguments, refusals that come before the device is asked for -- in the words desc_gcw_batch_create gives -- and
create without a device.  The CSR kernel has no size cap, so there is no host/device decision to test."""
import ctypes as C

import numpy as np
import pytest

from desc_amd.algorithms import marshal_edges
from tests.helpers import make_problem

SYMBOLS = ["desc_problem_batch_create", "desc_problem_batch_from_models", "desc_problem_batch_sizes", "desc_problem_batch_fetch",
           "desc_problem_batch_built_where", "desc_problem_batch_bytes", "desc_problem_batch_destroy", "desc_gcw_batch_create_on",
           "desc_refine_batch_create_on", "desc_pgd_batch_create_on", "desc_gcw_batch_bytes", "desc_refine_batch_bytes",
           "desc_pgd_batch_bytes"]


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
    assert callable(desc_amd.ProblemBatch) and "ProblemBatch" in desc_amd.__all__
    assert callable(lib.ProblemBatch)


@pytest.mark.parametrize("csr", ["host", "device"])
def test_empty_set_is_legal_and_touches_no_device(lib, csr):
    """count == 0: no device is asked for (this passes on a machine without one), the handles created on it are empty too."""
    from desc_amd import DESC_batch, DESC_PGD_batch, DESC_refine_batch, GCW_batch, ProblemBatch, Spectral_batch, ConstantStepSize
    s = lib.ProblemBatch([], device=0, csr=csr)
    assert len(s) == 0 and s.n == 0 and s.m == 0 and s.bytes() == (0, 0)
    assert all(v.size == 0 for v in s.fetch(rij=True, csr=True).values())
    g, r = lib.GcwBatch(None, on=s), lib.RefineBatch(None, on=s)
    b = lib.Batch(None, lib.default_params(), on=s, where=lib.BUILD_DEVICE)
    for h in (g, r, b):
        assert h.count == 0 and h.bytes() == (0, 0)
    assert g.run()[0] == [] and r.run(np.zeros(0), np.zeros(0))[0] == []
    s.close()                                        # the handles outlive the set
    assert g.run()[0] == []
    for h in (g, r, b):
        h.destroy()
    with ProblemBatch([], csr=csr) as ps:
        ok = dict(iters=3, Gradient=ConstantStepSize(0.01), verbose=False)
        assert len(ps) == 0 and not ps.closed
        assert Spectral_batch(ps) == [] and GCW_batch(ps, []) == [] and DESC_refine_batch(ps, [], []) == []
        assert DESC_PGD_batch(ps, ok) == [] and DESC_batch(ps, ok, build="device") == []
    assert ps.closed


def test_null_arguments(lib):
    L = lib.load()
    h = C.c_void_p(1)
    assert L.desc_problem_batch_create(None, 0, 0, lib.BUILD_HOST, None) == lib.ERR_INVALID
    assert L.desc_problem_batch_create(None, 1, 0, lib.BUILD_HOST, C.byref(h)) == lib.ERR_INVALID and not h.value
    h = C.c_void_p(1)
    assert L.desc_problem_batch_create(None, 0, 0, 7, C.byref(h)) == lib.ERR_INVALID and not h.value
    assert b"csr_where = 7" in L.desc_last_error()
    h = C.c_void_p(1)
    assert L.desc_problem_batch_from_models(None, C.byref(h)) == lib.ERR_INVALID and not h.value
    assert L.desc_problem_batch_from_models(None, None) == lib.ERR_INVALID
    p = lib.default_params()
    for rc in (L.desc_gcw_batch_create_on(None, 0, C.byref(h)), L.desc_refine_batch_create_on(None, C.byref(h)),
               L.desc_pgd_batch_create_on(None, C.byref(p), None, lib.BUILD_HOST, C.byref(h)),
               L.desc_problem_batch_sizes(None, None, None, None), L.desc_problem_batch_fetch(None, None, None, None, None, None, None),
               L.desc_problem_batch_bytes(None, None, None), L.desc_problem_batch_built_where(None),
               L.desc_gcw_batch_bytes(None, None, None), L.desc_refine_batch_bytes(None, None, None), L.desc_pgd_batch_bytes(None, None, None)):
        assert rc == lib.ERR_INVALID
    empty = lib.ProblemBatch([])
    assert L.desc_gcw_batch_create_on(empty.handle, 0, None) == lib.ERR_INVALID
    h = C.c_void_p(1)
    assert L.desc_gcw_batch_create_on(empty.handle, 9, C.byref(h)) == lib.ERR_INVALID and not h.value      # eig, in create_where's words
    assert b"eig = 9 is none of" in L.desc_last_error()
    h = C.c_void_p(1)
    assert L.desc_pgd_batch_create_on(empty.handle, C.byref(p), None, 5, C.byref(h)) == lib.ERR_INVALID and not h.value
    assert b"where = 5" in L.desc_last_error()
    assert L.desc_pgd_batch_create_on(empty.handle, None, None, lib.BUILD_HOST, C.byref(h)) == lib.ERR_INVALID
    L.desc_problem_batch_destroy(None)               # as free(NULL)


@pytest.mark.parametrize("csr", ["host", "device"])
def test_invalid_problems_are_refused_in_gcw_batch_creates_words(lib, csr):
    """Before the device is asked for: the refusal is the same with and without a GPU, and it is desc_gcw_batch_create's message."""
    mo, *_ = make_problem("uniform", n=20, p=0.5, seed=1)
    good = _arrays(lib, mo)
    eye2 = np.tile(np.eye(3).reshape(-1), 2)
    bad = dict(empty=lib.ProblemArrays(3, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)),
               unsorted=lib.ProblemArrays(3, np.array([1, 0], np.int32), np.array([2, 1], np.int32), eye2),
               loop=lib.ProblemArrays(3, np.array([0, 1], np.int32), np.array([1, 1], np.int32), eye2),
               out_of_range=lib.ProblemArrays(3, np.array([0, 1], np.int32), np.array([1, 3], np.int32), eye2),
               no_rij=lib.ProblemArrays(3, np.array([0, 1], np.int32), np.array([1, 2], np.int32)))
    for name, q in bad.items():
        with pytest.raises(lib.DescError) as e_gcw:
            lib.GcwBatch([good, q])
        with pytest.raises(lib.DescError) as e_set:
            lib.ProblemBatch([good, q], csr=csr)
        words = str(e_gcw.value).split(": ", 1)[1]
        assert "problem 1: " in words and e_set.value.code == e_gcw.value.code == lib.ERR_INVALID, name
        assert str(e_set.value).split(": ", 1)[1] == words, name
    arr = (lib.Problem * 2)(good.c, bad["empty"].c)
    h = C.c_void_p(1)
    assert lib.load().desc_problem_batch_create(arr, 2, 0, lib.CSR_WHERE[csr], C.byref(h)) == lib.ERR_INVALID and not h.value


@pytest.mark.parametrize("csr", ["host", "device"])
def test_create_without_a_device_fails_with_err_hip(lib, csr):
    if lib.load().desc_device_count() > 0:
        pytest.skip("a GPU is visible")
    mo, *_ = make_problem("uniform", n=20, p=0.5, seed=1)
    prob = _arrays(lib, mo)
    with pytest.raises(lib.DescError) as ei:
        lib.ProblemBatch([prob, prob], csr=csr)
    assert ei.value.code == lib.ERR_HIP and "no HIP device visible" in str(ei.value)
    h = C.c_void_p(1)
    rc = lib.load().desc_problem_batch_create(C.byref(prob.c), 1, 0, lib.CSR_WHERE[csr], C.byref(h))
    assert rc == lib.ERR_HIP and not h.value and lib.load().desc_last_error()


def test_problem_batch_refusals_are_value_errors(lib, monkeypatch):
    from desc_amd import (CEMP_batch, DESC_batch, DESC_init_batch, DESC_PGD_batch, DESC_refine_batch, GCW_batch, IRLS_GM_batch, MST_batch,
                          ProblemBatch, Spectral_batch, linprog_sij_batch, ConstantStepSize)
    mo, *_ = make_problem("uniform", n=20, p=0.5, seed=1)
    for bad in (mo, 7, None, np.zeros(3), "ab"):
        with pytest.raises(ValueError, match="sequence"):
            ProblemBatch(bad)
    for bad in ("gpu", "", None, 1):
        with pytest.raises(ValueError, match="csr must be 'host' or 'device'"):
            ProblemBatch([mo], csr=bad)
    for bad in (-1, 0.5, True, "0"):
        with pytest.raises(ValueError, match="device must be a non-negative integer"):
            ProblemBatch([mo], device=bad)

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(lib, "ProblemBatch", no_device)
    empty = (np.zeros((0, 2)), np.zeros((3, 3, 0)))
    with pytest.raises(ValueError, match="problem 1: empty edge list"):
        ProblemBatch([mo, empty])
    with pytest.raises(ValueError, match="problem 1: "):
        ProblemBatch([mo, 7])
    monkeypatch.undo()
    # a device that differs from the set's: every family, before anything else happens (the empty set needs no device)
    ps = ProblemBatch([], device=0)
    ok = dict(iters=3, Gradient=ConstantStepSize(0.01), verbose=False, device=1)
    cemp = dict(max_iter=1, reweighting=[1.0], nsample=5, device=1)
    calls = [lambda: Spectral_batch(ps, device=1), lambda: GCW_batch(ps, [], device=1), lambda: DESC_refine_batch(ps, [], [], device=1),
             lambda: DESC_PGD_batch(ps, ok), lambda: DESC_init_batch(ps, ok), lambda: DESC_batch(ps, ok), lambda: CEMP_batch(ps, cemp),
             lambda: MST_batch(ps, [], device=1), lambda: IRLS_GM_batch(ps, device=1), lambda: linprog_sij_batch(ps, dict(device=1))]
    for call in calls:
        with pytest.raises(ValueError, match=r"device = 1 differs from the device of the ProblemBatch \(0\)"):
            call()
    ps.close()
    with pytest.raises(ValueError, match="the ProblemBatch is closed"):
        Spectral_batch(ps)

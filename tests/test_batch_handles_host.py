"""CPU tests (no GPU) of what the five batched entry points share (desc_amd/csrc/batch_device.h, _lib._BatchHandle): the argument
checks of create, create or run without a device -- each call in its own words -- and the empty batch."""
import ctypes as C

import numpy as np
import pytest

from desc_amd.algorithms import marshal_edges
from tests import graph_shapes as gs

KINDS = ["pgd", "gcw", "cemp", "refine", "mst"]
# the refusal of a machine without a device names the call
NO_DEVICE = {"pgd": "no HIP device visible: DESC_PGD_batch has no CPU fallback",
             "gcw": "no HIP device visible: the batched eigen-solve has no CPU fallback",
             "cemp": "no HIP device visible: the batched CEMP has no CPU fallback",
             "refine": "no HIP device visible: the batched refinement has no CPU fallback",
             "mst": "no HIP device visible: the batched tree step has no CPU fallback"}


def problem(lib):
    mo = gs.band(8, 2, seed=1)
    n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None and n == 8
    return lib.ProblemArrays(n, ii, jj, rij)


def c_create(lib, kind, arr, count, out, device=0):
    """The raw create call of a handle kind (for "mst", which has no handle, the run call); returns its code."""
    L = lib.load()
    if kind == "pgd":
        p = lib.default_params()
        p.device = device
        return L.desc_pgd_batch_create(arr, count, C.byref(p), None, out)
    if kind == "gcw":
        return L.desc_gcw_batch_create(arr, count, device, out)
    if kind == "cemp":
        return L.desc_cemp_batch_create(arr, count, 10, 0, None, device, out)
    if kind == "refine":
        return L.desc_refine_batch_create(arr, count, device, out)
    m = sum(arr[b].m for b in range(max(count, 0))) if arr is not None else 0
    n = sum(arr[b].n for b in range(max(count, 0))) if arr is not None else 0
    S, R = np.full(max(m, 1), 0.5), np.zeros(9 * max(n, 1))
    return L.desc_mst_batch_run(arr, count, lib.ptr(S, lib.F64P), device, lib.ptr(R, lib.F64P), None, None)


def py_create(lib, kind, probs, device=0):
    """The same through _lib's owners; returns the handle (None for "mst")."""
    if kind == "pgd":
        p = lib.default_params()
        p.device = device
        return lib.Batch(probs, p)
    if kind == "gcw":
        return lib.GcwBatch(probs, device)
    if kind == "cemp":
        return lib.CempBatch(probs, 10, device=device)
    if kind == "refine":
        return lib.RefineBatch(probs, device)
    lib.mst_batch_run(probs, np.full(sum(q.m for q in probs), 0.5), device)
    return None


@pytest.mark.parametrize("kind", KINDS)
def test_create_checks_its_arguments(lib, kind):
    prob = problem(lib)
    arr = (lib.Problem * 1)(prob.c)
    for a, count in ((arr, -1), (None, 1)):
        h = C.c_void_p(1)
        assert c_create(lib, kind, a, count, C.byref(h)) == lib.ERR_INVALID
        assert "NULL argument or negative count" in lib.load().desc_last_error().decode()
        if kind != "mst":
            assert not h.value
    if kind != "mst":
        assert c_create(lib, kind, arr, 1, None) == lib.ERR_INVALID
        assert "out is NULL" in lib.load().desc_last_error().decode()


@pytest.mark.parametrize("kind", KINDS)
def test_no_device_is_err_hip_in_the_calls_own_words(lib, kind):
    assert len(set(NO_DEVICE.values())) == len(KINDS)
    if lib.load().desc_device_count() > 0:
        pytest.skip("a GPU is visible")
    prob = problem(lib)
    with pytest.raises(lib.DescError) as ei:
        py_create(lib, kind, [prob])
    assert ei.value.code == lib.ERR_HIP and NO_DEVICE[kind] in str(ei.value)
    h = C.c_void_p(1)
    assert c_create(lib, kind, (lib.Problem * 1)(prob.c), 1, C.byref(h)) == lib.ERR_HIP
    assert NO_DEVICE[kind] in lib.load().desc_last_error().decode()
    if kind != "mst":
        assert not h.value


@pytest.mark.parametrize("kind", KINDS)
def test_empty_batch_runs_twice_and_is_destroyed_twice(lib, kind):
    if kind == "mst":
        for _ in range(2):
            outs, timings = lib.mst_batch_run([], np.zeros(0))
            assert outs == [] and timings["ms_total"] == 0
        return
    b = py_create(lib, kind, [])
    assert b.count == 0 and b.m == 0 and (b.m_cycle if kind == "pgd" else b.n) == 0
    for _ in range(2):
        if kind == "pgd":
            outs, timings = b.run(lib.default_params())
        elif kind == "gcw":
            outs, timings = b.run()
        elif kind == "cemp":
            outs, timings = b.run([1.0, 2.0], 3)
        else:
            outs, timings = b.run(np.zeros(0), np.zeros(0))
        assert outs == [] and timings["ms_structure"] >= 0 and timings["ms_upload"] == 0
    b.destroy()
    assert b.handle is None
    b.destroy()

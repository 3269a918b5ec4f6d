"""CPU tests (no GPU) of the four batched creates that take a problem list and make their own resident set from it
(desc_gcw_batch_create, desc_refine_batch_create, desc_cemp_batch_create, desc_irls_batch_create): the order of the refusals -- a
family's size cap is refused per problem, between the other refusals of that problem; CEMP's degree cap and its sample budget after
every problem was validated -- all before any device call; a machine without a device in the family's own words; the empty batch."""
import ctypes as C

import numpy as np
import pytest

from desc_amd.algorithms import marshal_edges
from tests import graph_shapes as gs

KINDS = ["gcw", "refine", "cemp", "irls"]
NO_DEVICE = {"gcw": "no HIP device visible: the batched eigen-solve has no CPU fallback",
             "refine": "no HIP device visible: the batched refinement has no CPU fallback",
             "cemp": "no HIP device visible: the batched CEMP has no CPU fallback",
             "irls": "no HIP device visible: the batched IRLS has no CPU fallback"}
UNSORTED = "Ind is not strictly sorted by (i,j) at row 1 (DESC_PGD.m:5 requires it)"


def arrays(lib, mo):
    n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None
    return lib.ProblemArrays(n, ii, jj, rij)


def path(lib, n):
    ii = np.arange(n - 1, dtype=np.int32)
    return lib.ProblemArrays(n, ii, ii + 1, np.tile(np.eye(3).reshape(-1), n - 1))


def unsorted(lib):
    """A triangle whose second row comes before its first in (i, j) order."""
    return lib.ProblemArrays(3, np.array([0, 0, 1], np.int32), np.array([2, 1, 2], np.int32), np.tile(np.eye(3).reshape(-1), 3))


def c_create(lib, kind, probs, nsample=10):
    """The raw C create of a handle kind on a list of ProblemArrays -> (code, message, handle value)."""
    L = lib.load()
    arr = (lib.Problem * max(len(probs), 1))(*[q.c for q in probs])
    h = C.c_void_p(1)
    if kind == "gcw":
        rc = L.desc_gcw_batch_create_where(arr, len(probs), 0, lib.GCW_EIG["lds"], C.byref(h))
    elif kind == "refine":
        rc = L.desc_refine_batch_create(arr, len(probs), 0, C.byref(h))
    elif kind == "cemp":
        rc = L.desc_cemp_batch_create(arr, len(probs), nsample, 0, None, 0, C.byref(h))
    else:
        rc = L.desc_irls_batch_create(arr, len(probs), None, 0, C.byref(h))
    return rc, L.desc_last_error().decode(), h.value


def py_create(lib, kind, probs):
    return {"gcw": lambda: lib.GcwBatch(probs), "refine": lambda: lib.RefineBatch(probs), "cemp": lambda: lib.CempBatch(probs, 10),
            "irls": lambda: lib.IrlsBatch(probs)}[kind]()


@pytest.mark.parametrize("kind", ["gcw", "refine", "irls"])
def test_a_size_cap_is_refused_between_the_refusals_of_its_problem(lib, kind):
    """Problem 0 above the family's cap, problem 1 invalid: the cap of problem 0 is refused, problem 1 is never looked at.  Swapped:
    problem 0's unsorted row is refused, the cap of problem 1 is never reached."""
    cap, what, instead = {"gcw": (lib.gcw_batch_max_n(), "the 3n x 6 blocks of the eigen-solve", "GCW / DESC_init"),
                          "refine": (lib.refine_batch_max_n(), "the per-node state of the refinement", "DESC"),
                          "irls": (lib.irls_batch_max_n(), "the per-node state of the L1 stage", "IRLS_GM / IRLS_L12")}[kind]
    big, bad = path(lib, cap + 1), unsorted(lib)
    rc, msg, h = c_create(lib, kind, [big, bad])
    assert rc == lib.ERR_INVALID and not h
    assert f"problem 0: n = {cap + 1} exceeds {cap} ({what} must fit the LDS of one workgroup): solve it with {instead}" in msg
    rc, msg, h = c_create(lib, kind, [bad, big])
    assert rc == lib.ERR_INVALID and not h and f"problem 0: {UNSORTED}" in msg


def test_cemp_refuses_a_hub_after_every_problem_was_validated(lib):
    """CEMP's cap is one on a CSR row, which exists once every problem was validated: an invalid problem is refused first wherever it
    stands; a hub next to valid problems is refused, naming its problem and node."""
    cap = lib.cemp_batch_max_degree()
    hub, bad, ok = arrays(lib, gs.star(cap + 2, 1, seed=3)), unsorted(lib), path(lib, 5)
    rc, msg, h = c_create(lib, "cemp", [hub, bad])
    assert rc == lib.ERR_INVALID and not h and f"problem 1: {UNSORTED}" in msg
    rc, msg, h = c_create(lib, "cemp", [bad, hub])
    assert rc == lib.ERR_INVALID and not h and f"problem 0: {UNSORTED}" in msg
    for probs, b in (([hub, ok], 0), ([ok, hub], 1)):
        rc, msg, h = c_create(lib, "cemp", probs)
        assert rc == lib.ERR_INVALID and not h
        assert f"problem {b}: node 0 has {cap + 1} neighbours, more than the {cap} the batched sampler stages per row: solve it with CEMP" in msg


def test_cemp_refuses_a_sample_budget_of_2_to_the_31_before_any_device_call(lib):
    """m_total * nsample >= 2^31: DESC_ERR_TOO_LARGE with and without a device, and the largest budget below it gets as far as the device."""
    q = arrays(lib, gs.band(8, 2, seed=1))
    assert q.m == 13
    nsample = -(-2 ** 31 // (2 * q.m))                                   # two problems: 26 * nsample >= 2^31 > 26 * (nsample - 1)
    assert 2 * q.m * nsample >= 2 ** 31 > 2 * q.m * (nsample - 1)
    rc, msg, h = c_create(lib, "cemp", [q, q], nsample)
    assert rc == lib.ERR_TOO_LARGE and not h
    assert f"the batch holds 26 edges with {nsample} samples each: m_total * nsample exceeds 2^31, split the batch" in msg
    rc, msg, h = c_create(lib, "cemp", [q, unsorted(lib)], nsample)       # an invalid problem still comes first
    assert rc == lib.ERR_INVALID and not h and f"problem 1: {UNSORTED}" in msg
    if lib.load().desc_device_count() <= 0:
        rc, msg, h = c_create(lib, "cemp", [q, q], nsample - 1)
        assert rc == lib.ERR_HIP and not h and NO_DEVICE["cemp"] in msg


@pytest.mark.parametrize("kind", KINDS)
def test_no_device_is_err_hip_in_the_familys_own_words(lib, kind):
    assert len(set(NO_DEVICE.values())) == len(KINDS)
    if lib.load().desc_device_count() > 0:
        pytest.skip("a GPU is visible")
    q = arrays(lib, gs.band(8, 2, seed=1))
    with pytest.raises(lib.DescError) as ei:
        py_create(lib, kind, [q])
    assert ei.value.code == lib.ERR_HIP and NO_DEVICE[kind] in str(ei.value)
    rc, msg, h = c_create(lib, kind, [q])
    assert rc == lib.ERR_HIP and not h and NO_DEVICE[kind] in msg
    assert "the resident problem set" not in msg and "the resident problem set" not in str(ei.value)


@pytest.mark.parametrize("kind", KINDS)
def test_empty_batch_moves_no_byte_runs_twice_and_is_destroyed_twice(lib, kind):
    b = py_create(lib, kind, [])
    assert b.count == 0 and b.n == 0 and b.m == 0 and b.bytes() == (0, 0)
    for _ in range(2):
        if kind == "gcw":
            outs, timings = b.run()
        elif kind == "cemp":
            outs, timings = b.run([1.0, 2.0], 3)
        elif kind == "refine":
            outs, timings = b.run(np.zeros(0), np.zeros(0))
        else:
            outs, timings = b.run(lib.IRLS_GM)
        assert outs == [] and timings["ms_structure"] >= 0 and timings["ms_upload"] == 0
        assert b.bytes() == (0, 0)
    b.destroy()
    assert b.handle is None
    b.destroy()

"""CPU tests (no GPU) of the batched IRLS's host side (desc_irls_batch_*, _lib.IrlsBatch, IRLS_GM_batch / IRLS_L12_batch): ABI surface,
the size cap, refusals that come before any device call and name the problem, the empty batch, and the host-built spanning-tree
sequence against a NumPy restatement of Utils/BoxMedianSO3Graph.m:79-114."""
import ctypes as C

import numpy as np
import pytest

from tests import graph_shapes as gs
from tests import irls_batch_cases as cases

SYMBOLS = ["desc_irls_batch_max_n", "desc_irls_batch_create", "desc_irls_batch_sizes", "desc_irls_batch_run", "desc_irls_batch_destroy",
           "desc_irls_tree_sequence"]


def test_abi_surface(lib):
    import desc_amd
    L = lib.load()
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/desc_amd.h").read()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS and name + "(" in hdr, name
    assert C.sizeof(lib.IrlsBatchTimings) == 40      # as include/desc_amd.h states: 5 doubles
    assert "} desc_irls_batch_timings;    /* 40 bytes */" in hdr
    assert [f for f, _ in lib.IrlsBatchTimings._fields_] == ["ms_structure", "ms_upload", "ms_project", "ms_solve", "ms_total"]
    assert C.sizeof(lib.IrlsInfo) == 16 + 8 + 16 + 8 * 4 + 8 + 7 * 8      # desc_irls_info: one record per problem
    for name in ("IRLS_GM_batch", "IRLS_L12_batch"):
        assert callable(getattr(desc_amd, name)) and name in desc_amd.__all__
    assert issubclass(lib.IrlsBatch, lib._BatchHandle) and lib.IrlsBatch._kind == "irls"


def test_size_cap(lib):
    cap = lib.irls_batch_max_n()
    assert cap == lib.load().desc_irls_batch_max_n() >= 278 == lib.gcw_batch_max_n()      # what the other rotation calls accept is accepted here
    assert 8 * 34 * cap + 12 * 1024 <= 160 * 1024 < 8 * 34 * (cap + 1) + 12 * 1024        # 34 doubles per node next to the kernel's fixed LDS


def test_refusals_come_before_any_device_call(lib, monkeypatch):
    from desc_amd import IRLS_GM, IRLS_GM_batch, IRLS_L12, IRLS_L12_batch

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(lib, "IrlsBatch", no_device)
    ok = cases.problems()[0]
    Ind, Rij = ok
    cap = lib.irls_batch_max_n()
    for fn in (IRLS_GM_batch, IRLS_L12_batch):
        for bad in (7, None, np.zeros(3), "ab", iter([ok])):
            with pytest.raises(ValueError, match="sequence"):
                fn(bad)
        with pytest.raises(ValueError, match="problem 1: empty edge list"):
            fn([ok, (np.zeros((0, 2)), np.zeros((3, 3, 0)))])
        for mi in ((10,), (1, 2, 3), 5):
            with pytest.raises(ValueError, match="MaxIterations must have two entries"):
                fn([ok], MaxIterations=mi)
        with pytest.raises(ValueError, match="problem 1: the quaternion form"):
            fn([ok, (Ind, np.zeros((4, Ind.shape[0])))])
        # two components: nodes 1-16 and 17-32
        two = (np.concatenate([Ind, Ind + 16]), np.concatenate([Rij, Rij], axis=2))
        with pytest.raises(ValueError, match="problem 2: the graph is not connected") as ei:
            fn([ok, ok, two])
        assert "solve it with IRLS_GM / IRLS_L12" in str(ei.value)
        # a node id that no edge touches counts as a component
        with pytest.raises(ValueError, match="problem 0: the graph is not connected"):
            fn([(Ind + 1, Rij)])
        with pytest.raises(ValueError, match=f"problem 1: n = {cap + 1} exceeds {cap}") as ei:
            fn([ok, gs.band(cap + 1, 1, seed=2)])
        assert "solve it with IRLS_GM / IRLS_L12" in str(ei.value)
        # a pair given as (j, i): the library's input rule, in the single call's words
        with pytest.raises(ValueError) as e_single:
            {IRLS_GM_batch: IRLS_GM, IRLS_L12_batch: IRLS_L12}[fn](cases.flipped(2)[1], cases.flipped(2)[0])
        with pytest.raises(ValueError) as e_batch:
            fn([ok, cases.flipped(2)])
        assert str(e_batch.value) == "problem 1: " + str(e_single.value) and "Ind(:,1) < Ind(:,2)" in str(e_single.value)
        with pytest.raises(TypeError):
            fn([ok], Rinit=np.zeros((3, 3, 16)))       # there is no Rinit
        assert fn([]) == [] and fn([], return_info=True) == []


def test_c_entry_points_refuse_before_the_device(lib):
    """desc_irls_batch_create itself: the refusals of its host part carry DESC_ERR_INVALID and name the problem, whatever the device."""
    from desc_amd.algorithms import marshal_edges
    L = lib.load()
    Ind, Rij = cases.problems()[0]
    n, ii, jj, rij, _ = marshal_edges(Ind, Rij)
    ok = lib.ProblemArrays(n, ii, jj, rij)
    n2, i2, j2, r2, _ = marshal_edges(np.concatenate([Ind, Ind + 16]), np.concatenate([Rij, Rij], axis=2))
    two = lib.ProblemArrays(n2, i2, j2, r2)
    h = C.c_void_p()
    arr = lib._problem_array([ok, two])
    assert L.desc_irls_batch_create(arr, 2, None, 99, C.byref(h)) == lib.ERR_INVALID and not h.value
    assert b"problem 1: the graph is not connected (16 of 32 nodes reached" in L.desc_last_error()
    bad = np.zeros(ok.m, dtype=np.int32)               # no permutation
    orders = (lib.I32P * 1)(lib.ptr(bad, lib.I32P))
    assert L.desc_irls_batch_create(lib._problem_array([ok]), 1, orders, 99, C.byref(h)) == lib.ERR_INVALID and not h.value
    assert b"problem 0: order must be a permutation" in L.desc_last_error()
    assert L.desc_irls_batch_create(None, 1, None, 0, C.byref(h)) == lib.ERR_INVALID
    assert L.desc_irls_batch_run(None, 0, 5.0, 10, 100, None, None, None, None) == lib.ERR_INVALID
    assert b"NULL handle" in L.desc_last_error()
    assert L.desc_irls_batch_sizes(None, None, None, None) == lib.ERR_INVALID


def test_empty_handle_runs_and_returns_nothing(lib):
    b = lib.IrlsBatch([])
    assert b.count == 0
    for mode in (lib.IRLS_GM, lib.IRLS_L12):
        outs, timings = b.run(mode)
        assert outs == [] and timings["ms_solve"] == 0 and timings["ms_project"] == 0
    with pytest.raises(lib.DescError, match="mode must be") as ei:
        b.run(7)
    assert ei.value.code == lib.ERR_INVALID
    b.destroy()


def tree_sequence_numpy(Ind):
    """Utils/BoxMedianSO3Graph.m:79-114, the graph part, on the caller's rows (1-based Ind with i < j or j < i as given): passes over
    the rows in order from node 1; a row with exactly one end reached reaches the other.  Returns per reached node (row, direction):
    direction 0 sets Q(j) from Q(i), 1 sets Q(i) from Q(j), with (i, j) = (min, max) of the row as IRLS_GM.m sorts them."""
    Ind = np.asarray(Ind)
    i_all, j_all = Ind.min(axis=1), Ind.max(axis=1)
    n = int(Ind.max())
    done = np.zeros(n + 1, dtype=bool)
    done[1] = True
    out = []
    while done[1:].sum() < n:
        span = False
        for row in range(Ind.shape[0]):
            i, j = int(i_all[row]), int(j_all[row])
            if done[i] and not done[j]:
                out.append((row, 0)); done[j] = True; span = True
            if not done[i] and done[j]:
                out.append((row, 1)); done[i] = True; span = True
        assert span, "not connected"
    return out, done


@pytest.mark.parametrize("name", ["shuffled40", "path", "sorted16"])
def test_tree_sequence_is_the_reference_s_pass_over_the_caller_s_rows(lib, name):
    from desc_amd.algorithms import marshal_edges
    Ind, Rij = {"shuffled40": lambda: cases.shuffled(2), "path": cases.path_graph, "sorted16": lambda: cases.problems()[0]}[name]()
    n, ii, jj, rij, perm = marshal_edges(Ind, Rij)
    assert (perm is None) == (name == "sorted16")
    prob = lib.ProblemArrays(n, ii, jj, rij)
    edges, dirs, reached = lib.irls_tree_sequence(prob, perm)
    assert reached == n and edges.size == n - 1
    rows = edges if perm is None else perm[edges]                                 # sorted edge id -> the caller's row
    ref, done = tree_sequence_numpy(Ind)
    assert done[1:].all()
    assert [(int(r), int(d)) for r, d in zip(rows, dirs)] == ref                  # identical sequences
    new = np.where(dirs == 0, jj[edges], ii[edges])                               # the node each entry sets
    assert sorted(new.tolist()) == list(range(1, n))                              # every node but the root exactly once
    if name == "path":
        assert rows.tolist() == list(range(n - 2, -1, -1)) and not dirs.any()     # one node per pass, from the far end of the list
    if name == "shuffled40":
        e0, d0, _ = lib.irls_tree_sequence(prob, None)                            # the sorted order gives another tree
        assert not (np.array_equal(e0, edges) and np.array_equal(d0, dirs))

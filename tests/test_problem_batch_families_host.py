"""CPU tests (no GPU) of the CEMP, MST, MPLS and IRLS handles on a resident problem set (desc_cemp_batch_create_on,
desc_irls_batch_create_on, desc_mst_batch_run_on): ABI surface, NULL sets, the empty set, and the two host checks that the set's calls
run on index-only problems (no rotations) -- the same answers and the same words as on full problems."""
import ctypes as C

import numpy as np
import pytest

from desc_amd.algorithms import marshal_edges
from tests import graph_shapes as gs
from tests.helpers import make_problem

SYMBOLS = ["desc_cemp_batch_create_on", "desc_irls_batch_create_on", "desc_mst_batch_run_on", "desc_cemp_batch_bytes", "desc_irls_batch_bytes"]


def test_abi_surface(lib):
    L = lib.load()
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/desc_amd.h").read()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS and name + "(" in hdr, name
    assert callable(lib.mst_batch_run_on)


def test_a_null_set_is_refused(lib):
    L = lib.load()
    h = C.c_void_p(1)
    assert L.desc_cemp_batch_create_on(None, 5, 0, None, C.byref(h)) == lib.ERR_INVALID and not h.value
    h = C.c_void_p(1)
    assert L.desc_irls_batch_create_on(None, None, C.byref(h)) == lib.ERR_INVALID and not h.value
    assert L.desc_mst_batch_run_on(None, None, None, None, None, None) == lib.ERR_INVALID
    assert L.desc_cemp_batch_bytes(None, None, None) == lib.ERR_INVALID and L.desc_irls_batch_bytes(None, None, None) == lib.ERR_INVALID
    empty = lib.ProblemBatch([])
    assert L.desc_cemp_batch_create_on(empty.handle, 5, 0, None, None) == lib.ERR_INVALID        # out is NULL
    h = C.c_void_p(1)
    assert L.desc_cemp_batch_create_on(empty.handle, 0, 0, None, C.byref(h)) == lib.ERR_INVALID and not h.value
    assert b"need nsample >= 1" in L.desc_last_error()                                           # desc_cemp_batch_create's words
    empty.close()


@pytest.mark.parametrize("csr", ["host", "device"])
def test_empty_set_gives_empty_handles_without_a_device(lib, csr):
    """count == 0: no device is asked for (this passes on a machine without one)."""
    import desc_amd as D
    s = lib.ProblemBatch([], device=0, csr=csr)
    c, i = lib.CempBatch(None, 5, 0, None, on=s), lib.IrlsBatch(None, None, on=s)
    for h in (c, i):
        assert h.count == 0 and h.n == 0 and h.m == 0 and h.bytes() == (0, 0)
    assert c.run([1.0], 2)[0] == [] and i.run(lib.IRLS_GM, max_iter_l1=1, max_iter_irls=1)[0] == []
    assert c.mpls_run(np.zeros(0), np.zeros(0), 1e-3, 2, [1.0], [0.9], [1.0])[0] == []
    outs, _, moved = lib.mst_batch_run_on(s, np.zeros(0), return_bytes=True)
    assert outs == [] and moved == (0, 0)
    s.close()                                        # the handles outlive the set
    assert c.run([1.0], 1)[0] == [] and i.run(lib.IRLS_L12)[0] == []
    with pytest.raises(ValueError, match="the ProblemBatch is closed"):
        lib.mst_batch_run_on(s, np.zeros(0))
    with pytest.raises(ValueError, match="the ProblemBatch is closed"):
        lib.CempBatch(None, 5, on=s)
    for h in (c, i):
        h.destroy()
    cemp = dict(max_iter=1, reweighting=[1.0], nsample=5)
    mpls = dict(stop_threshold=1e-3, max_iter=1, reweighting=[1.0], thresholding=[0.95], cycle_info_ratio=[1.0])
    with D.ProblemBatch([], csr=csr) as ps:
        assert D.CEMP_batch(ps, cemp) == [] and D.CEMP_GCW_batch(ps, cemp) == [] and D.MST_batch(ps, []) == []
        assert D.CEMP_MST_batch(ps, cemp) == [] and D.MPLS_batch(ps, cemp, mpls) == []
        assert D.IRLS_GM_batch(ps) == [] and D.IRLS_L12_batch(ps) == []


def _both(lib, mo):
    """A problem with its rotations and the same problem with its endpoints alone, and the marshalling's permutation."""
    n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    return lib.ProblemArrays(n, ii, jj, rij), lib.ProblemArrays(n, ii, jj), perm


def _path(lib, n):
    """The path on n nodes, with and without (identity) rotations."""
    ii = np.arange(n - 1, dtype=np.int32)
    return lib.ProblemArrays(n, ii, ii + 1, np.tile(np.eye(3).reshape(-1), n - 1)), lib.ProblemArrays(n, ii, ii + 1)


def _words(lib, fn, *args):
    with pytest.raises(lib.DescError) as e:
        fn(*args)
    assert e.value.code == lib.ERR_INVALID
    return str(e.value)


def test_mst_batch_check_on_index_only_problems(lib):
    good = [_both(lib, make_problem("uniform", n=n, p=0.5, seed=s)[0]) for n, s in ((20, 1), (33, 2))]
    lib.mst_batch_check([f for f, _, _ in good])
    lib.mst_batch_check([x for _, x, _ in good])
    split = _both(lib, gs.model("two_components"))
    full = _words(lib, lib.mst_batch_check, [good[0][0], split[0]])
    assert "problem 1: the graph is disconnected: 2 components" in full
    assert _words(lib, lib.mst_batch_check, [good[0][1], split[1]]) == full
    cap = lib.mst_batch_max_n()
    big = _path(lib, cap + 1)
    full = _words(lib, lib.mst_batch_check, [good[1][0], good[0][0], big[0]])
    assert f"problem 2: n = {cap + 1} exceeds {cap} (the per-node keys of the tree kernel must fit the LDS of one workgroup): solve it with MST / MPLS" in full
    assert _words(lib, lib.mst_batch_check, [good[1][1], good[0][1], big[1]]) == full
    lib.mst_batch_check([_path(lib, cap)[1]])        # the cap itself is taken
    empty = lib.ProblemArrays(3, np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert "problem 1: empty edge list" in _words(lib, lib.mst_batch_check, [good[0][1], empty])


def test_irls_tree_sequence_on_index_only_problems(lib):
    mo = make_problem("uniform", n=33, p=0.4, seed=2)[0]
    perm = np.random.default_rng(5).permutation(mo.Ind.shape[0])
    shuffled = type("M", (), dict(Ind=mo.Ind[perm], RijMat=np.asfortranarray(mo.RijMat[:, :, perm])))
    for m in (mo, shuffled, gs.model("two_components")):
        full, index, order = _both(lib, m)
        want, got = lib.irls_tree_sequence(full, order), lib.irls_tree_sequence(index, order)
        assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]) and want[2] == got[2]
        assert (want[2] == full.n) == (m is not gs.model("two_components"))
    full, index, _ = _both(lib, mo)
    bad = np.zeros(full.m, dtype=np.int32)
    assert _words(lib, lib.irls_tree_sequence, full, bad) == _words(lib, lib.irls_tree_sequence, index, bad)
    assert "order must be a permutation of 0..m-1" in _words(lib, lib.irls_tree_sequence, index, bad)


def test_the_python_side_caps_on_index_only_problems(lib):
    """What the set's calls check before they ask for a handle, in the list path's words."""
    from desc_amd.algorithms import _check_batch_sizes, _check_cemp_batch_degrees, _check_mst_batch
    cap = lib.irls_batch_max_n()
    full, index = _path(lib, cap + 1)
    for q in (full, index):
        with pytest.raises(ValueError, match=rf"problem 0: n = {cap + 1} exceeds {cap} \(the per-node state of the L1 stage must fit the LDS"):
            _check_batch_sizes([q], cap, "per-node state of the L1 stage", "IRLS_GM / IRLS_L12")
        _check_cemp_batch_degrees([q])
        _check_mst_batch([q])
    split = _both(lib, gs.model("two_components"))
    for q in split[:2]:
        with pytest.raises(ValueError, match="problem 0: the graph is disconnected: 2 components"):
            _check_mst_batch([q])

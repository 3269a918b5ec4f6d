"""CPU tests (no GPU) of the batched rotation alignment (desc_align_batch_*, Rotation_Alignment_batch): ABI surface, the refusals that
come before any device call, the empty batch, the conditioning of the cases tests/test_gpu_align_batch.py runs, and the NumPy restatement
(tests/align_batch_oracle.py) against Rotation_Alignment's LAPACK SVD on all of them.

Conditioning.  No case is left out of the LAPACK comparison: every problem's gap (s2 + sign(det A) s3) / s1 is at least GAP_MIN = 1e-2
(the smallest is 0.033, a garbage problem of n = 5).  The constant cases are pairs of rotations, so their A = n E'G has three equal
singular values (gap 2); the two-class cases' pairs were chosen (by their seeds, tests/align_batch_cases.py) so that the gap is 0.5."""
import ctypes as C

import numpy as np
import pytest

from tests import align_batch_cases as cases
from tests import align_batch_oracle as O
from tests.align_batch_cases import EXACT_MAX, MEASURED

SYMBOLS = ["desc_align_batch_create", "desc_align_batch_sizes", "desc_align_batch_run", "desc_align_batch_destroy", "desc_test_align_project"]


def test_abi_surface(lib):
    import desc_amd
    L = lib.load()
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/desc_amd.h").read()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS and name + "(" in hdr, name
    assert C.sizeof(lib.AlignBatchTimings) == 32                                             # as include/desc_amd.h states
    assert callable(desc_amd.Rotation_Alignment_batch) and "Rotation_Alignment_batch" in desc_amd.__all__
    assert issubclass(lib.AlignBatch, lib._BatchHandle) and callable(lib.hook_align_project)


def test_python_refusals_come_before_any_device_call(lib, monkeypatch, capsys):
    from desc_amd import Rotation_Alignment_batch as RAB

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(lib, "AlignBatch", no_device)
    E, G = cases.SINGLE["noisy-3"]
    for bad in (None, 7, E, "ab"):
        with pytest.raises(ValueError, match="R_est_list must be a sequence"):
            RAB(bad, [G])
        with pytest.raises(ValueError, match="R_gt_list must be a sequence"):
            RAB([E], bad)
    with pytest.raises(ValueError, match="R_est_list holds 2 problems, R_gt_list 1"):
        RAB([E, E], [G])
    for bad in (np.zeros((3, 3)), np.zeros((3, 3, 0)), np.zeros((3, 4, 2)), np.zeros((2, 3, 3)), "x", None, np.zeros((3, 3, 2, 1))):
        with pytest.raises(ValueError, match="problem 1: R_est must be"):
            RAB([E, bad], [G, G])
        with pytest.raises(ValueError, match="problem 0: R_gt must be"):
            RAB([E, E], [bad, G])
    with pytest.raises(ValueError, match="problem 1: R_est has n = 2, R_gt n = 3"):
        RAB([E, E[:, :, :2]], [G, G])
    for val in (np.nan, np.inf, -np.inf):
        bad = E.copy()
        bad[1, 2, 1] = val
        with pytest.raises(ValueError, match="problem 1: R_est of node 2 is not finite"):
            RAB([E, bad], [G, G])
        with pytest.raises(ValueError, match="problem 0: R_gt of node 2 is not finite"):
            RAB([E, E], [bad, G])
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="device"):
            RAB([E], [G], device=bad)
    assert RAB([], []) == [] and RAB((), (), rotations=False, return_info=True) == []
    assert capsys.readouterr().out == ""


def _create(lib, n, R_gt, count=None, out="ref"):
    n = np.asarray(n, dtype=np.int32)
    h = C.c_void_p(1)
    rc = lib.load().desc_align_batch_create(lib.ptr(n, lib.I32P), lib.ptr(R_gt, lib.F64P), len(n) if count is None else count, 0,
                                            C.byref(h) if out == "ref" else None)
    return rc, h, lib.load().desc_last_error().decode()


def test_c_entry_point_refuses_before_the_device(lib):
    """DESC_ERR_INVALID / DESC_ERR_TOO_LARGE naming the problem, and *out stays NULL.  Without a GPU a call that reached the device would
    return DESC_ERR_HIP instead; with one, the message is the same."""
    L = lib.load()
    gt = np.concatenate([cases.SINGLE["noisy-3"][1].reshape(-1, order="F"), cases.SINGLE["noisy-2"][1].reshape(-1, order="F")])
    for bad in (0, -4):
        rc, h, msg = _create(lib, [3, bad], gt)
        assert rc == lib.ERR_INVALID and not h.value and f"problem 1: n = {bad}, need n >= 1" in msg, msg
    for val in (np.nan, np.inf):
        x = gt.copy()
        x[9 * 3 + 9 * 1 + 4] = val
        rc, h, msg = _create(lib, [3, 2], x)
        assert rc == lib.ERR_INVALID and not h.value and "problem 1: R_gt of node 2 is not finite" in msg, msg
    # 9 N >= 2^31: refused from the sizes alone, before R_gt is read (the buffer here holds five blocks)
    big = (2 ** 31 + 8) // 9
    rc, h, msg = _create(lib, [3, big - 3], gt)
    assert rc == lib.ERR_TOO_LARGE and not h.value and "problem 1" in msg, msg
    rc, h, msg = _create(lib, [2 ** 31 - 1, 2 ** 31 - 1, 5], gt)
    assert rc == lib.ERR_TOO_LARGE and not h.value and "problem 0" in msg, msg
    # NULL arguments and a negative count
    rc, h, _ = _create(lib, [3, 2], gt, count=-1)
    assert rc == lib.ERR_INVALID and not h.value
    rc, h, _ = _create(lib, [3, 2], None)
    assert rc == lib.ERR_INVALID and not h.value
    h = C.c_void_p(1)
    assert L.desc_align_batch_create(None, lib.ptr(gt, lib.F64P), 2, 0, C.byref(h)) == lib.ERR_INVALID and not h.value
    assert _create(lib, [3, 2], gt, out=None)[0] == lib.ERR_INVALID
    out = np.zeros(9)
    assert L.desc_align_batch_run(None, lib.ptr(gt, lib.F64P), None, lib.ptr(out, lib.F64P), None, lib.ptr(out, lib.F64P), lib.ptr(out, lib.F64P),
                                  None) == lib.ERR_INVALID
    assert L.desc_align_batch_sizes(None, None, None) == lib.ERR_INVALID
    assert L.desc_test_align_project(lib.ptr(out, lib.F64P), -1, 0, lib.ptr(out, lib.F64P)) == lib.ERR_INVALID
    assert L.desc_test_align_project(None, 1, 0, lib.ptr(out, lib.F64P)) == lib.ERR_INVALID
    assert L.desc_test_align_project(lib.ptr(out, lib.F64P), 1, 0, None) == lib.ERR_INVALID
    with pytest.raises(ValueError, match="R_gt must hold"):
        lib.AlignBatch([3, 2], gt[:-1])


def test_create_without_a_device_fails_with_err_hip(lib):
    if lib.load().desc_device_count() > 0:
        pytest.skip("a GPU is visible")
    E, G = cases.SINGLE["noisy-3"]
    with pytest.raises(lib.DescError) as ei:
        lib.AlignBatch([3], G.reshape(-1, order="F"))
    assert ei.value.code == lib.ERR_HIP
    rc, h, msg = _create(lib, [3], G.reshape(-1, order="F"))
    assert rc == lib.ERR_HIP and not h.value and "no CPU fallback" in msg
    with pytest.raises(lib.DescError) as ei:
        lib.hook_align_project(np.eye(3).reshape(1, 9))
    assert ei.value.code == lib.ERR_HIP


def test_empty_batch_through_the_c_abi(lib):
    b = lib.AlignBatch([], np.zeros(0))
    assert b.count == 0 and b.n == 0 and b.node_off.tolist() == [0]
    for rotations in (True, False):
        arrays, timings = b.run(np.zeros(0), rotations=rotations)
        assert all(v is None or v.size == 0 for v in arrays.values()) and (arrays["R_out"] is None) == (not rotations)
        assert set(timings) == {"ms_upload", "ms_align", "ms_copy", "ms_total"} and timings["ms_align"] == 0
    b.destroy()
    assert lib.hook_align_project(np.zeros((0, 9))).shape == (0, 9)


def test_the_cases_are_well_conditioned():
    """The cap on cases left out of the LAPACK comparison is zero; det A < 0 occurs among the garbage problems of n = 3 and n = 7."""
    negative = set()
    for name, E, G in cases.every_problem():
        A, gap = cases.gram(E, G)
        assert gap >= cases.GAP_MIN, (name, gap)
        if np.linalg.det(A) < 0:
            negative.add(name.rsplit("-", 1)[0] if name.count("-") == 2 else name)
    assert {"garbage-3", "garbage-7"} <= negative
    assert [E.shape[2] for E, _ in cases.MIXED] == [1, 257, 2, 100, 64] and len(cases.MANY) == 300
    assert all(E.flags.f_contiguous and G.flags.f_contiguous and E.shape == G.shape for _, E, G in cases.every_problem())


def test_restatement_against_lapack():
    """The restated projection (and with it the whole restated call) against Rotation_Alignment on every case.  MEASURED holds what this
    comparison gave on the CPU the tolerances of the GPU test were derived on; another CPU's LAPACK kernels round differently, hence
    the factor 4 (a quarter of the GPU test's margin)."""
    refs = list(cases.reference("single")) + list(cases.reference("mixed")) + list(cases.reference("many"))
    worst = dict.fromkeys(MEASURED, 0.0)
    for (name, E, G), (R_out, R_align, mean, median, err) in zip(cases.every_problem(), refs):
        o_out, o_align, o_mean, o_median, o_err = O.rotation_alignment(E, G)
        assert np.abs(o_align.T @ o_align - np.eye(3)).max() <= 1e-13 and abs(np.linalg.det(o_align) - 1) <= 1e-13, name
        big = err > 1e-3
        d = dict(R_align=np.abs(o_align - R_align).max(), R_out=np.abs(o_out - R_out).max(), err=np.abs(o_err - err)[big].max(initial=0.0))
        if median > 1e-3:
            d.update(mean=abs(o_mean - mean), median=abs(o_median - median))
        else:                                                     # an exact problem: both answers lie in [0, EXACT_MAX]
            assert 0 <= o_mean <= EXACT_MAX and 0 <= o_median <= EXACT_MAX and o_err.max() <= EXACT_MAX, name
        for k, v in d.items():
            worst[k] = max(worst[k], float(v))
        assert o_median == float(np.median(o_err)) or E.shape[2] % 2 == 0, name
    print("restatement against Rotation_Alignment, max over the cases:", worst)
    for k in MEASURED:
        assert worst[k] <= 4 * MEASURED[k], (k, worst[k])


def test_restated_orders_on_hand_checkable_input():
    assert O.median_error([5.0]) == 5.0 and O.median_error([1.0, 4.0]) == 2.5 and O.median_error([3.0, 1.0, 2.0]) == 2.0
    assert O.median_error([2.0, 2.0, 2.0, 7.0]) == 2.0 and O.median_error([1.0, 2.0, 2.0, 7.0, 9.0, 2.0]) == 2.0
    assert O.mean_error(np.arange(1.0, 601.0)) == 300.5                                     # integers: every order gives the same sum
    x = np.random.default_rng(3).random(1000)
    assert abs(O.mean_error(x) - x.mean()) <= 1e-15 and O.mean_error(x[:1]) == x[0]
    # the butterfly gives every lane of a wave the same total
    v = np.random.default_rng(4).random(256)
    w = v.copy()
    for s in (1, 2, 7, 15, 16, 32):
        w = w + w[np.arange(256) ^ s]
    assert all(np.unique(w[k:k + 64]).size == 1 for k in (0, 64, 128, 192))
    # the projection: a rotation is its own projection, a reflection moves to the nearest rotation
    R = cases.haar(np.random.default_rng(5), 1)[0]
    assert np.abs(O.project(R) - R).max() <= 1e-15
    assert np.abs(O.project(np.diag([3.0, 2.0, -1.0])) - np.diag([1.0, 1.0, 1.0])).max() <= 1e-15
    assert np.abs(O.project(np.diag([-3.0, 2.0, 1.0])) - np.diag([-1.0, 1.0, -1.0])).max() <= 1e-15

"""CPU tests (no GPU) of the batched MPLS's host side (desc_mpls_batch_*, CempBatch.mpls_run, MPLS_batch): ABI surface, the size cap,
refusals that come before any device call and name the problem, the empty batch."""
import ctypes as C

import numpy as np
import pytest

from tests import cemp_batch_cases
from tests import graph_shapes as gs
from tests import mpls_batch_cases as cases

SYMBOLS = ["desc_mpls_batch_max_n", "desc_mpls_batch_run"]


def test_abi_surface(lib):
    import desc_amd
    L = lib.load()
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/desc_amd.h").read()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS and name + "(" in hdr, name
    assert C.sizeof(lib.MplsBatchTimings) == 40      # as include/desc_amd.h states: 5 doubles
    assert "} desc_mpls_batch_timings;    /* 40 bytes */" in hdr
    assert [f for f, _ in lib.MplsBatchTimings._fields_] == ["ms_setup", "ms_input", "ms_loop", "ms_download", "ms_total"]
    assert callable(desc_amd.MPLS_batch) and "MPLS_batch" in desc_amd.__all__
    assert callable(lib.CempBatch.mpls_run)


def test_size_cap_is_the_refinement_s(lib):
    L = lib.load()
    assert L.desc_mpls_batch_max_n() == L.desc_refine_batch_max_n()
    assert lib.mpls_batch_max_n() == lib.refine_batch_max_n() == 748
    assert 8 * 26 * lib.mpls_batch_max_n() + 8 * 1024 <= 160 * 1024      # the per-node state and the kernel's fixed LDS fit one workgroup


def test_refusals_come_before_any_device_call(lib, monkeypatch):
    from desc_amd import CEMP_MST_batch, MPLS_batch
    mo = cases.models()[1]
    cemp, mpls = cases.demo_params()

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    for name in ("CempBatch", "mst_batch_run"):
        monkeypatch.setattr(lib, name, no_device)
    # what CEMP_MST_batch refuses, in its words
    empty = (np.zeros((0, 2)), np.zeros((3, 3, 0)))
    Ind2, R2 = cemp_batch_cases.two_triangles()
    dcap, tcap = lib.cemp_batch_max_degree(), lib.mst_batch_max_n()
    star, big = gs.star(dcap + 2, 1, seed=3), gs.band(tcap + 1, 1, seed=2)
    for args, kw in ((([mo, empty], cemp), {}), (([mo, mo], cemp), dict(seeds=[1])), (([mo], dict(cemp, nsample=0)), {}),
                     (([mo], dict(cemp, max_iter=-1)), {}), (([mo], dict(cemp, reweighting=[])), {}),
                     (([mo], {k: v for k, v in cemp.items() if k != "reweighting"}), {}), (([mo, star], cemp), {}), (([mo, big], cemp), {}),
                     (([(Ind2, R2), mo], cemp), {})):
        with pytest.raises(ValueError) as e_init:
            CEMP_MST_batch(*args, **kw)
        with pytest.raises(ValueError) as e_batch:
            MPLS_batch(*args, mpls, **kw)
        assert str(e_batch.value) == str(e_init.value)
    for bad in (mo, 7, None, np.zeros(3), "ab"):
        with pytest.raises(ValueError, match="sequence"):
            MPLS_batch(bad, cemp, mpls)
    # the loop's own parameters
    for name in ("reweighting", "thresholding", "cycle_info_ratio"):
        with pytest.raises(ValueError, match=f"MPLS_parameters.{name} needs at least one entry"):
            MPLS_batch([mo], cemp, dict(mpls, **{name: []}))
        with pytest.raises(ValueError, match=f"MPLS_parameters.{name} is required"):
            MPLS_batch([mo], cemp, {k: v for k, v in mpls.items() if k != name})
    for name in ("stop_threshold", "max_iter"):
        with pytest.raises(ValueError, match=f"MPLS_parameters.{name} is required"):
            MPLS_batch([mo], cemp, {k: v for k, v in mpls.items() if k != name})
    # the size cap: connected, within the sampler's and the tree kernel's caps
    cap = lib.mpls_batch_max_n()
    assert cap < tcap
    with pytest.raises(ValueError, match=f"problem 1: n = {cap + 1} exceeds {cap}") as ei:
        MPLS_batch([mo, gs.band(cap + 1, 1, seed=2)], cemp, mpls)
    assert "solve it with MPLS" in str(ei.value)
    assert MPLS_batch([], cemp, mpls) == []
    assert MPLS_batch([], cemp, mpls, return_info=True) == []


def test_c_entry_point_refuses_a_null_handle(lib):
    L = lib.load()
    one = (C.c_double * 1)(1.0)
    assert L.desc_mpls_batch_run(None, None, None, 1e-3, 100, one, 1, one, 1, one, 1, None, None, None) == lib.ERR_INVALID
    assert b"NULL handle" in L.desc_last_error()


def test_empty_handle_runs_and_returns_nothing(lib):
    b = lib.CempBatch([], 10)
    assert b.count == 0
    outs, timings = b.mpls_run(np.zeros(0), np.zeros(0), 1e-3, 100, [32.0], [0.9], [0.5])
    assert outs == [] and timings["ms_loop"] == 0 and timings["ms_setup"] == 0
    outs, _ = b.run([1.0], 3)                           # the two runs may alternate
    assert outs == []
    outs, _ = b.mpls_run(np.zeros(0), np.zeros(0), 1e-3, 2, [32.0], [0.9], [0.5])
    assert outs == []
    with pytest.raises(lib.DescError, match="need >= 1 entry each") as ei:
        b.mpls_run(np.zeros(0), np.zeros(0), 1e-3, 100, [32.0], [], [0.5])
    assert ei.value.code == lib.ERR_INVALID
    b.destroy()

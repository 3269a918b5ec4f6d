"""CPU tests (no GPU) of the streamed eigen-solve's host side (desc_gcw_batch_create_where, the ``eig`` keyword of Spectral_batch,
GCW_batch, DESC_init_batch, DESC_batch, CEMP_GCW_batch and linprog_sij_batch): ABI surface, the two caps, the refusals that come
before any device call, the conditioning of the GPU tests' inputs."""
import ctypes as C

import pytest

from desc_amd import ConstantStepSize
from desc_amd.algorithms import marshal_edges
from tests import gcw_batch_cases as cases
from tests import gcw_streamed_cases as streamed
from tests import graph_shapes as gs
from tests.helpers import make_problem

NEW_SYMBOLS = ["desc_gcw_batch_create_where", "desc_gcw_batch_streamed_max_n"]
CEMP_PAR = dict(max_iter=3, reweighting=[1.0, 2.0, 4.0], nsample=10)


def _arrays(lib, mo):
    n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None
    return lib.ProblemArrays(n, ii, jj, rij)


def test_abi_surface(lib):
    L = lib.load()
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/desc_amd.h").read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS and name + "(" in hdr, name
    for name, value in (("DESC_GCW_EIG_LDS", 0), ("DESC_GCW_EIG_STREAMED", 1), ("DESC_GCW_EIG_AUTO", 2)):
        assert any(line.split() == ["#define", name, str(value)] for line in hdr.splitlines()), name
    assert lib.GCW_EIG == dict(lds=0, streamed=1, auto=2)
    assert C.sizeof(lib.SpectralInfo) == 56          # the kernel that ran is reported through the reserved field: the record keeps its size


def test_caps(lib):
    assert lib.gcw_batch_max_n() == 278              # the default has not moved
    c = lib.gcw_batch_streamed_max_n()
    # ONE 3n x 6 block of doubles and 448 doubles of small matrices within the 160 KiB a workgroup may declare; one more node does not fit
    assert (18 * c + 448) * 8 <= 160 * 1024 < (18 * (c + 1) + 448) * 8
    assert c >= lib.refine_batch_max_n()             # the streamed eigen-solve starts every problem the refinement takes


def test_refusals_come_before_any_device_call(lib, monkeypatch):
    from desc_amd import CEMP_GCW_batch, DESC_batch, DESC_init_batch, GCW_batch, Spectral_batch, linprog_sij_batch
    mo, *_ = make_problem("uniform", n=20, p=0.5, seed=1)
    S = gs.noisy_truth(mo, 1)
    cap, c, rcap = lib.gcw_batch_max_n(), lib.gcw_batch_streamed_max_n(), lib.refine_batch_max_n()
    assert rcap == 748

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    for name in ("GcwBatch", "Batch", "RefineBatch", "CempBatch", "LpBatch"):
        monkeypatch.setattr(lib, name, no_device)
    ok = dict(iters=3, Gradient=ConstantStepSize(0.01), verbose=False)
    calls = {
        "Spectral_batch": lambda mos, **k: Spectral_batch(mos, **k),
        "GCW_batch": lambda mos, **k: GCW_batch(mos, [gs.noisy_truth(m, 3) for m in mos], **k),
        "DESC_init_batch": lambda mos, **k: DESC_init_batch(mos, ok, **k),
        "DESC_batch": lambda mos, **k: DESC_batch(mos, ok, **k),
        "CEMP_GCW_batch": lambda mos, **k: CEMP_GCW_batch(mos, CEMP_PAR, **k),
        "linprog_sij_batch": lambda mos, **k: linprog_sij_batch(mos, **k),
    }
    # an unknown eig: every call names the three values
    for name, call in calls.items():
        for bad in ("global", "LDS", "", None, 1):
            with pytest.raises(ValueError, match='eig must be "lds", "streamed" or "auto"'):
                call([mo], eig=bad)
    # one node past the streamed cap, as problem 1
    over = gs.band(c + 1, 1, seed=2)
    for name, call in calls.items():
        for eig in ("auto", "streamed"):
            with pytest.raises(ValueError, match=f"problem 1: n = {c + 1} exceeds {c} ") as ei:
                call([mo, over], eig=eig)
            assert "streamed eigen-solve" in str(ei.value), name
    # DESC_batch and the LP row: the refinement's cap, before the PGD and the eigen-solve
    big = gs.band(rcap + 1, 1, seed=3)
    for name in ("DESC_batch", "linprog_sij_batch"):
        for eig in ("auto", "streamed"):
            with pytest.raises(ValueError, match=f"problem 1: n = {rcap + 1} exceeds {rcap} \\(the per-node state of the refinement"):
                calls[name]([mo, big], eig=eig)
    # the default, spelled or not, refuses n = 279 with the text it had
    b279 = gs.band(cap + 1, 1, seed=2)
    text = f"problem 1: n = {cap + 1} exceeds {cap} \\(the 3n x 6 blocks of the eigen-solve must fit the LDS of one workgroup\\): solve it with "
    for name, call in calls.items():
        for kw in ({}, dict(eig="lds")):
            with pytest.raises(ValueError, match=text):
                call([mo, b279], **kw)
    with pytest.raises(ValueError, match=text + "GCW / DESC_init"):
        GCW_batch([mo, b279], [S, gs.noisy_truth(b279, 2)])
    with pytest.raises(ValueError, match=text + "linprog_sij, or pass rotations=False for S_vec alone"):
        linprog_sij_batch([mo, b279])


def test_create_where_refuses_before_the_device(lib):
    """The C entry point: DESC_ERR_INVALID naming the problem -- the same message with and without a GPU -- and *out stays NULL."""
    mo, *_ = make_problem("uniform", n=20, p=0.5, seed=1)
    cap, c = lib.gcw_batch_max_n(), lib.gcw_batch_streamed_max_n()
    L = lib.load()
    small = _arrays(lib, mo)
    one = (lib.Problem * 1)(small.c)
    h = C.c_void_p(1)
    for bad in (3, -1, 99):
        h = C.c_void_p(1)
        assert L.desc_gcw_batch_create_where(one, 1, 0, bad, C.byref(h)) == lib.ERR_INVALID and not h.value
        assert f"eig = {bad}" in L.desc_last_error().decode()
    probs = [small, _arrays(lib, gs.band(c + 1, 1, seed=2))]
    arr = (lib.Problem * 2)(*[q.c for q in probs])
    for eig in (lib.GCW_EIG["streamed"], lib.GCW_EIG["auto"]):
        h = C.c_void_p(1)
        assert L.desc_gcw_batch_create_where(arr, 2, 0, eig, C.byref(h)) == lib.ERR_INVALID and not h.value
        assert f"problem 1: n = {c + 1} exceeds {c} " in L.desc_last_error().decode()
    with pytest.raises(lib.DescError, match=f"problem 1: n = {c + 1} exceeds {c} ") as ei:
        lib.GcwBatch(probs, eig="streamed")
    assert ei.value.code == lib.ERR_INVALID
    # the LDS mode through the new entry point is desc_gcw_batch_create: its cap and its words
    probs = [small, _arrays(lib, gs.band(cap + 1, 1, seed=2))]
    arr = (lib.Problem * 2)(*[q.c for q in probs])
    h = C.c_void_p(1)
    assert L.desc_gcw_batch_create_where(arr, 2, 0, lib.GCW_EIG["lds"], C.byref(h)) == lib.ERR_INVALID and not h.value
    msg = L.desc_last_error().decode()
    assert f"problem 1: n = {cap + 1} exceeds {cap} (the 3n x 6 blocks of the eigen-solve" in msg and "GCW / DESC_init" in msg
    with pytest.raises(ValueError, match="eig must be"):
        lib.GcwBatch([small], eig="global")
    # an empty batch opens no device in any mode
    for eig in ("lds", "streamed", "auto"):
        b = lib.GcwBatch([], eig=eig)
        assert b.count == 0 and b.run(s_vec=[])[0] == []
        b.destroy()


def test_every_input_of_the_gpu_tests_is_well_conditioned():
    """No case of tests/test_gpu_gcw_streamed.py may be left out for conditioning: every gap is at least 1e-2."""
    gaps = {}
    for name in streamed.BIG:
        mo, S = streamed.big(name)
        gaps[name] = (cases.gcw_gap(mo, S), streamed.spectral_gap(mo))
    for k, (mo, S) in enumerate(zip(streamed.composite_models(), streamed.composite_S())):
        gaps[f"composite{k}"] = (cases.gcw_gap(mo, S), streamed.spectral_gap(mo))
    print(gaps)
    for name, (g, s) in gaps.items():
        assert g >= 1e-2 and s >= 1e-2, (name, g, s)
    assert streamed.big("U1112")[0].Ind.max() == 1112
    for name, want in (("U279", (0.162, 0.53)), ("U400", (0.610, 0.85)), ("U748", (0.052, 0.34)), ("U1112", (0.054, 0.34))):
        assert abs(gaps[name][0] - want[0]) < 1e-3 and abs(gaps[name][1] - want[1]) < 1e-2, (name, gaps[name])

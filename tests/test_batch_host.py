"""CPU tests (no GPU) of the batched solver's host side: ABI surface, refusals that need no device, the concatenation of the
per-problem structures against the oracle's."""
import ctypes as C

import numpy as np
import pytest

from desc_amd import ConstantStepSize, HybridGradient
from tests.helpers import make_problem

# the mixed batch of tests/test_gpu_batch.py: (n, p, model seed)
MIXED = [(12, 0.6, 9), (40, 0.5, 10), (90, 0.5, 8), (150, 0.95, 6), (200, 0.5, 4)]
BATCH_SYMBOLS = ["desc_pgd_batch_create", "desc_pgd_batch_sizes", "desc_pgd_batch_get_structure", "desc_pgd_batch_get_s0",
                 "desc_pgd_batch_run", "desc_pgd_batch_destroy", "desc_pgd_batch_concat"]


class _Counting:
    """A plugin of the caller's own: DESC_PGD_batch must refuse it without calling it."""
    calls = 0

    def GetStep(self, g):
        self.calls += 1
        return -0.01 * g


def test_batch_abi_surface(lib):
    L = lib.load()
    for name in BATCH_SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS, name
    assert C.sizeof(lib.BatchResult) == 104          # as include/desc_amd.h states: 8 pointers + 5 doubles
    assert lib.BatchResult.iters_run.offset == 48 and lib.BatchResult.ms_structure.offset == 64


def test_batch_create_without_a_device_fails_with_err_hip(lib):
    if lib.load().desc_device_count() > 0:
        pytest.skip("a GPU is visible")
    mo, nn, ii, jj, rij = make_problem("uniform", n=20, p=0.5, seed=1)
    with pytest.raises(lib.DescError) as ei:
        lib.Batch([lib.ProblemArrays(nn, ii, jj, rij)] * 2, lib.default_params())
    assert ei.value.code == lib.ERR_HIP
    assert len(str(ei.value)) > len("desc_amd error -2: ")
    # the C entry point itself leaves *out NULL
    prob = lib.ProblemArrays(nn, ii, jj, rij)
    h = C.c_void_p(1)
    p = lib.default_params()
    rc = lib.load().desc_pgd_batch_create(C.byref(prob.c), 1, C.byref(p), None, C.byref(h))
    assert rc == lib.ERR_HIP and not h.value and lib.load().desc_last_error()


def test_batch_refusals_come_before_any_device_call(lib, monkeypatch):
    from desc_amd import DESC_PGD_batch
    mo, *_ = make_problem("uniform", n=20, p=0.5, seed=1)

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(lib, "Batch", no_device)
    ok = dict(iters=3, Gradient=ConstantStepSize(0.01), verbose=False)
    plug = _Counting()
    with pytest.raises(ValueError, match="GetStep"):
        DESC_PGD_batch([mo], dict(ok, Gradient=plug))
    assert plug.calls == 0
    with pytest.raises(ValueError, match="make_plots"):
        DESC_PGD_batch([mo], dict(ok, make_plots=True, ErrVec=mo.ErrVec, R_orig=mo.R_orig))
    with pytest.raises(ValueError, match="seeds"):
        DESC_PGD_batch([mo, mo], ok, seeds=[1, 2, 3])
    for bad in (mo, 7, None, np.zeros(3), "ab"):
        with pytest.raises(ValueError, match="sequence"):
            DESC_PGD_batch(bad, ok)
    with pytest.raises(ValueError, match="problem 1"):
        DESC_PGD_batch([mo, (mo.Ind,)], ok)
    assert DESC_PGD_batch([], ok) == []
    assert DESC_PGD_batch((), dict(ok, Gradient=HybridGradient(0.001, 0.9, 0.999, 10)), return_info=True) == []


def test_empty_batch_through_the_c_abi(lib):
    b = lib.Batch([], lib.default_params())
    assert b.count == 0 and b.m == 0 and b.m_cycle == 0
    outs, timings = b.run(lib.default_params())
    assert outs == []
    b.destroy()


def test_n_sample_above_64_is_refused_without_a_device(lib):
    """(310, 0.95, seed 7): n_sample = 70.  The refusal names the problem and the value and comes before the device is asked for --
    so it is the same message with and without a GPU."""
    from desc_amd import DESC_PGD_batch
    small, nn, ii, jj, rij = make_problem("uniform", n=20, p=0.5, seed=1)
    big, bn, bi, bj, br = make_problem("uniform", n=310, p=0.95, q=0.2, sigma=0.1, seed=7)
    p = lib.default_params(); p.seed = 3
    with pytest.raises(lib.DescError) as ei:
        lib.Batch([lib.ProblemArrays(nn, ii, jj, rij), lib.ProblemArrays(bn, bi, bj, br)], p)
    assert ei.value.code == lib.ERR_INVALID
    assert "problem 1" in str(ei.value) and "n_sample = 70" in str(ei.value) and "DESC_PGD" in str(ei.value)
    with pytest.raises(ValueError, match="problem 1: n_sample = 70"):
        DESC_PGD_batch([small, big], dict(iters=3, Gradient=ConstantStepSize(0.01), seed=3, verbose=False))


def test_concatenation_equals_numpy_concatenation_of_the_oracle_structures(lib, oracle):
    """desc_pgd_batch_concat (offsets, globalised indices; -1 stays -1) on the library's per-problem structures against a NumPy
    concatenation of the oracle's structures of the same problems, each built alone with local ids."""
    sts, refs = [], []
    for n, pp, seed in MIXED:
        mo, nn, ii, jj, rij = make_problem("uniform", n=n, p=pp, q=0.2, sigma=0.1, seed=seed)
        sts.append(lib.Structure.build(lib.ProblemArrays(nn, ii, jj), 30, 1, lib.BUILD_HOST, 0))
        refs.append(oracle.build_structure(nn, ii, jj, seed=1))
    got = lib.batch_concat(sts)
    eo = np.concatenate([[0], np.cumsum([r["m"] for r in refs])])
    co = np.concatenate([[0], np.cumsum([r["m_cycle"] for r in refs])])
    so = np.concatenate([[0], np.cumsum([r["m_pos"] for r in refs])])
    assert np.array_equal(got["edge_off"], eo) and np.array_equal(got["cycle_off"], co) and np.array_equal(got["seg_off"], so)
    assert np.array_equal(got["pos_edge"], np.concatenate([r["pos_edge"] + eo[b] for b, r in enumerate(refs)]))
    assert np.array_equal(got["cum"], np.concatenate([r["cum_ind"][:-1] + co[b] for b, r in enumerate(refs)] + [[co[-1]]]))
    for key, off in (("e_jk", eo), ("e_ki", eo)):
        assert np.array_equal(got[key], np.concatenate([r[key] + off[b] for b, r in enumerate(refs)])), key
    for key in ("ikj", "jki"):
        want = np.concatenate([np.where(r[key] < 0, -1, r[key] + co[b]) for b, r in enumerate(refs)])
        assert np.array_equal(got[key], want), key
        assert (got[key] == -1).any()
    assert [int(np.diff(r["cum_ind"]).max()) for r in refs] == [5, 17, 30, 34, 30]      # all three lane-group widths
    for s in sts:
        s.free()

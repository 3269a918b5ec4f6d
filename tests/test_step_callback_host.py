"""User-defined params.Gradient plugins (any object with GetStep, DESC_PGD.m:207): what can be checked without a GPU -- the
translation into DESC_STEP_EXTERNAL, the validation of what GetStep returns, the loud failure without a device, and the host side
of desc_pgd_ext_begin / _grad / _apply under AddressSanitizer + UBSan against the mock HIP runtime."""
import os
import subprocess
import sys

import numpy as np
import pytest

from desc_amd import DESC, DESC_PGD, ConstantStepSize, HybridGradient, PiecewiseStepSize
from desc_amd import _lib
from desc_amd.algorithms import is_external, make_c_params
from tests.helpers import make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Momentum:
    def __init__(self, lr=0.01, mu=0.9):
        self.lr, self.mu, self.v, self.calls = lr, mu, None, 0

    def GetStep(self, grad):
        self.calls += 1
        self.v = -self.lr * grad if self.v is None else self.mu * self.v - self.lr * grad
        return self.v


class Wrapped:
    """Forwards to a known rule without being a subclass of it: takes the external path."""

    def __init__(self, g):
        self.g = g

    def GetStep(self, grad):
        return self.g.GetStep(grad)


def test_plugin_with_getstep_translates_to_external():
    p, G = make_c_params(dict(iters=5, Gradient=Momentum()))
    assert p.step_kind == _lib.STEP_EXTERNAL == 3 and p.t0 == 0 and p.iters == 5
    p, _ = make_c_params(dict(iters=5, Gradient=Wrapped(PiecewiseStepSize(0.1, 5))))
    assert p.step_kind == _lib.STEP_EXTERNAL
    assert is_external(Momentum()) and not is_external(ConstantStepSize(1.0))


def test_known_classes_and_their_subclasses_stay_native():
    class MyConstant(ConstantStepSize):
        pass

    class MyHybrid(HybridGradient):
        def GetStep(self, grad):          # a subclass goes native whatever it overrides, as isinstance always did
            raise AssertionError("not called")

    p, _ = make_c_params(dict(iters=3, Gradient=MyConstant(0.25)))
    assert (p.step_kind, p.lr) == (_lib.STEP_CONSTANT, 0.25)
    p, _ = make_c_params(dict(iters=3, Gradient=MyHybrid(0.01, 0.9, 0.99, 10)))
    assert p.step_kind == _lib.STEP_HYBRID
    assert not is_external(MyConstant(1.0))


def test_objects_without_a_callable_getstep_are_refused():
    class NotCallable:
        GetStep = 3

    with pytest.raises(TypeError, match="GetStep"):
        make_c_params(dict(iters=3, Gradient=object()))
    with pytest.raises(TypeError, match="GetStep"):
        make_c_params(dict(iters=3, Gradient=NotCallable()))
    with pytest.raises(TypeError):
        make_c_params(dict(iters=3, Gradient=lambda g: -g))          # a bare function is no handle object


def test_validate_step():
    ok = _lib.validate_step(np.zeros(7), 7)
    assert ok.shape == (7,) and ok.dtype == np.float64
    assert _lib.validate_step(np.zeros((1, 7)), 7).shape == (7,)                     # MATLAB's row vector
    assert _lib.validate_step(np.zeros(14)[::2], 7).flags.c_contiguous
    assert _lib.validate_step(np.full(3, np.nan), 3).shape == (3,)                   # non-finite values are the caller's business
    with pytest.raises(ValueError, match="7 entries"):
        _lib.validate_step(np.zeros(6), 7)                                           # wrong length
    with pytest.raises(ValueError, match="float64"):
        _lib.validate_step(np.zeros(7, dtype=np.float32), 7)                         # wrong dtype
    with pytest.raises(ValueError, match="float64"):
        _lib.validate_step(np.zeros(7, dtype=np.int64), 7)
    for bad in (None, 0.5, [0.0] * 7, (0.0,) * 7):
        with pytest.raises(ValueError, match="NumPy array"):
            _lib.validate_step(bad, 7)                                               # a non-array


def test_custom_plugin_without_gpu_fails_loudly():
    """No device: a custom plugin gets DescError like every other call -- never a silent result, and GetStep is never called."""
    if _lib.load().desc_device_count() > 0:
        pytest.skip("a GPU is visible")
    mo, nn, ii, jj, rij = make_problem("uniform", n=20, p=0.5, seed=1)
    G = Momentum()
    with pytest.raises(_lib.DescError):
        DESC_PGD(mo.Ind, mo.RijMat, dict(iters=3, Gradient=G, verbose=False))
    with pytest.raises(_lib.DescError):
        DESC_PGD(mo.Ind, mo.RijMat, dict(iters=3, Gradient=G, verbose=False), return_info=True)
    with pytest.raises(_lib.DescError):
        DESC(mo.Ind, mo.RijMat, dict(iters=3, Gradient=G, verbose=False))
    assert G.calls == 0


def test_step_kind_external_is_refused_by_the_one_call_paths():
    """desc_pgd_solve / desc_pgd_run cannot call back: DESC_STEP_EXTERNAL there is an argument error, before any device work."""
    mo, nn, ii, jj, rij = make_problem("uniform", n=20, p=0.5, seed=1)
    prob = _lib.ProblemArrays(nn, ii, jj, rij)
    p = _lib.default_params()
    p.iters = 3; p.step_kind = _lib.STEP_EXTERNAL; p.build_where = _lib.BUILD_HOST
    with pytest.raises(_lib.DescError) as e:
        _lib.solve(prob, p)
    assert _lib.load().desc_device_count() <= 0 or e.value.code == _lib.ERR_INVALID


def test_ext_calls_refuse_null_handles():
    L = _lib.load()
    g = np.zeros(4)
    assert L.desc_pgd_ext_begin(None, None) == _lib.ERR_INVALID
    assert L.desc_pgd_ext_grad(None, g.ctypes.data, _lib.MEM_HOST) == _lib.ERR_INVALID
    assert L.desc_pgd_ext_apply(None, g.ctypes.data, _lib.MEM_HOST, None, None, None) == _lib.ERR_INVALID
    assert b"NULL" in L.desc_last_error()


def test_host_side_of_the_stepping_calls_under_asan():
    """The sanitizer host build (tests/hipmock/build_host.py globs csrc/*.hip) still links and loads with the two-phase iteration in it,
    and the stepping calls -- every layout, call-order errors, host-mode copies into fenced buffers -- are clean under ASan + UBSan."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipmock"))
    import build_host
    rt = build_host.runtime_lib("address")
    if rt is None:
        pytest.skip("no address sanitizer runtime in this toolchain")
    so = build_host.build(ROOT, "address")
    env = dict(os.environ, LD_PRELOAD=rt, DESC_AMD_LIB=so, OPENBLAS_NUM_THREADS="1",
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hipmock", "drive_stepfn.py")], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    report = r.stdout[-3000:] + r.stderr[-6000:]
    assert r.returncode == 0, report
    assert "STEPFN HOSTSAN OK" in r.stdout, report
    for marker in ("ERROR: AddressSanitizer", "runtime error:"):
        assert marker not in r.stderr, report

"""Test infrastructure: drives the host side of the caller-supplied step rule (desc_pgd_ext_begin / _grad / _apply, Solver.run_external)
against the mock HIP runtime, every layout forced, with fenced caller buffers -- memory behaviour and call-order errors, not values
(kernels do not run under the mock).

Run by tests/test_step_callback_host.py in a subprocess with the sanitizer runtime preloaded."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ["DESC_DEBUG_GUARD"] = "1"
os.environ["DESC_CACHE_MB"] = "0"        # every "device" block fresh from calloc: the stop flag a kernel would have written reads back as 0

import numpy as np  # noqa: E402

from desc_amd import _lib as lib  # noqa: E402
from tests.helpers import c_params, make_problem  # noqa: E402

VAR = {"band": "3", "node": "2", "gather": "1"}


def expect_state(call):
    try:
        call()
    except lib.DescError as e:
        assert e.code == lib.ERR_STATE, (e.code, str(e))
    else:
        raise AssertionError("DESC_ERR_STATE expected")


def main():
    L = lib.load()
    assert hasattr(L, "hipmock_launch_count"), "this driver must run against the mock build"
    # segments of up to 32 cycles, of 65..256 (n_sample_min 100) and of more than 256 (n_sample_min 300: gather layout, multi-pass kernels)
    for n, p, nmin in ((60, 0.5, 30), (150, 0.9, 100), (330, 0.97, 300)):
        mo, nn, ii, jj, rij = make_problem("uniform", n=n, p=p, q=0.2, sigma=0.1, seed=3)
        prob = lib.ProblemArrays(nn, ii, jj, rij)
        for variant in ("band", "node", "gather"):
            os.environ["DESC_DEBUG_VARIANT"] = VAR[variant]
            try:
                st = lib.Structure.build(prob, nmin, 1, lib.BUILD_HOST, 0)
                s = lib.Solver(prob, st, 0)
                st.free()
            finally:
                os.environ.pop("DESC_DEBUG_VARIANT", None)
            mc = s.m_cycle
            g = lib.out_buffer(mc)
            pe = c_params(4, step_kind=lib.STEP_EXTERNAL, seed=1)
            expect_state(lambda: s.ext_grad(g))                     # before begin
            expect_state(lambda: s.ext_apply(g))
            s.ext_begin(pe)
            expect_state(lambda: s.ext_apply(g))                    # no gradient handed out yet
            expect_state(lambda: s.iterate(1))                      # the built-in rules are off while the caller steps
            for it in range(4):
                s.ext_grad(g)
                s.ext_apply(np.ascontiguousarray(-0.01 * g[:mc]))
                if it == 1:
                    s.download()                                    # between two iterations
            expect_state(lambda: s.ext_grad(g))                     # params.iters steps applied
            out = s.download(want_w=True)
            assert out["iters_run"] == 4 and out["t_end"] == 4 and out["obj"].shape == (4,) and out["w"].shape == (mc,)
            calls = []
            out = s.run_external(c_params(3, seed=1), lambda grad: calls.append(grad.size) or -0.5 * grad, want_w=True)
            assert calls == [mc] * 3 and out["iters_run"] == 3 and out["calls"] == 3
            s.run(c_params(3, seed=1))                              # back to a built-in rule on the same handle
            expect_state(lambda: s.ext_apply(g))
            s.destroy()
        print("ok", n, flush=True)
    # a sharded handle refuses all three calls
    mo, nn, ii, jj, rij = make_problem("uniform", n=90, p=0.5, q=0.2, sigma=0.1, seed=8)
    prob = lib.ProblemArrays(nn, ii, jj, rij)
    st = lib.Structure.build(prob, 30, 1, lib.BUILD_HOST, 0)
    s = lib.Solver(prob, st, 0, 0, 2)
    g = lib.out_buffer(s.m_cycle)
    expect_state(lambda: s.ext_begin(c_params(3, step_kind=lib.STEP_EXTERNAL, seed=1)))
    expect_state(lambda: s.ext_grad(g))
    expect_state(lambda: s.ext_apply(g))
    s.destroy(); st.free()
    # no cycle at all: empty vectors, the loop breaks at patience + 1
    prob = lib.ProblemArrays(4, np.array([0, 1, 2], dtype=np.int32), np.array([1, 2, 3], dtype=np.int32), np.tile(np.eye(3).reshape(-1), 3))
    st = lib.Structure.build(prob, 30, 1, lib.BUILD_HOST, 0)
    s = lib.Solver(prob, st, 0); st.free()
    out = s.run_external(c_params(100, seed=1), lambda grad: -grad)
    assert out["iters_run"] == 31 and out["calls"] == 31
    s.destroy()
    lib.verify_guards()
    lib.trim_memory()
    assert L.hipmock_live_blocks() == 0, "device blocks leaked"
    print("STEPFN HOSTSAN OK launches", L.hipmock_launch_count(), flush=True)


if __name__ == "__main__":
    main()

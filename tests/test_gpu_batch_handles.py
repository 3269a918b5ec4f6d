"""GPU tests of what the five batched entry points share (desc_amd/csrc/batch_device.h): the refusal of a device id past the last one,
and the timing events a handle owns from its first run to its destruction."""
import ctypes as C

import numpy as np
import pytest

from tests.test_batch_handles_host import KINDS, c_create, problem

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", KINDS)
def test_device_one_past_the_last_is_refused(lib, kind):
    ndev = lib.load().desc_device_count()
    assert ndev >= 1
    probs = [problem(lib), problem(lib)]
    h = C.c_void_p(1)
    rc = c_create(lib, kind, (lib.Problem * 2)(*[q.c for q in probs]), 2, C.byref(h), device=ndev)
    msg = lib.load().desc_last_error().decode()
    print(kind, rc, msg)
    assert rc == lib.ERR_INVALID and f"device {ndev} out of range (0..{ndev - 1})" in msg
    if kind != "mst":
        assert not h.value


def test_gcw_handle_gives_the_same_bits_on_every_run(lib):
    b = lib.GcwBatch([problem(lib), problem(lib)])
    runs = [b.run() for _ in range(3)]
    b.destroy()
    for outs, timings in runs:
        assert len(outs) == 2 and timings["ms_eig"] > 0
        for (R, info), (R0, info0) in zip(outs, runs[0][0]):
            assert info["converged"] and np.isfinite(R).all()
            assert np.array_equal(R, R0) and info["eigenvalues"] == info0["eigenvalues"] and info["iters"] == info0["iters"]

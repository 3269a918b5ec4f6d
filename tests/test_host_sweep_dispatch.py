"""The sweep dispatch of the PGD solver (sweep_gather.hip, sweep_node.hip, sweep_band.hip, pgd.hip, pgd_layout.hip) on the host side, without a GPU: the library built against the mock HIP runtime (tests/hipmock; kernels
do not run).  For every entry of the instance table of tests/test_gpu_sweep_instances.py the handle is created as the GPU case creates
it, two iterations are enqueued, and the instance the dispatch chose (desc_debug_last_sweep) and the prefix the handle reports
(desc_pgd_kernel_name) are compared with the table.  The GPU cases confirm the numbers; this confirms the choice."""
import functools
import json
import os
import subprocess
import sys

import pytest

from tests.test_gpu_sweep_instances import CASES, _case_id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import functools, json, os, sys
sys.path.insert(0, sys.argv[1])
from desc_amd import _lib as lib
from tests.helpers import c_params
from tests.test_gpu_sweep_instances import CASES, LAYOUTS, STEPS, _bands_env, _base, _case_id, _graph
assert hasattr(lib.load(), "hipmock_launch_count"), "must run against the mock build"

@functools.lru_cache(maxsize=None)
def structure(T):
    mo, nn, ii, jj, rij = _graph(_base(T))
    prob = lib.ProblemArrays(nn, ii, jj, rij)
    return prob, lib.Structure.build(prob, T, 0, lib.BUILD_HOST, 0)

out = {}
for case in CASES:
    layout, T, step, world, name = case
    env = dict(LAYOUTS[layout], **(_bands_env(layout, T) if world > 1 else {}))
    os.environ.update(env)
    try:
        prob, st = structure(T)
        p = c_params(2, seed=0, **STEPS[step])
        s = lib.Solver(prob, st, 0, 0, world)
        try:
            assert s.max_cnt == T, (s.max_cnt, T)
            if world == 1:
                s.reset(p); s.iterate(2)
            else:
                s.shard_bind(None, None, None)
                s.reset(p); s.shard_finish(1)
                for _ in range(2):
                    s.shard_colsum(); s.shard_sweep(); s.shard_finish(0)
            out[_case_id(case)] = dict(last=s.last_sweep(), kernel=s.kernel_name())
        finally:
            s.destroy()
    finally:
        for k in env:
            os.environ.pop(k, None)
print("RESULT " + json.dumps(out))
"""


@functools.lru_cache(maxsize=None)
def _dispatched():
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipmock"))
    import build_host
    so = build_host.build(ROOT, "none")
    env = dict(os.environ, DESC_AMD_LIB=so, DESC_CACHE_MB="0", OPENBLAS_NUM_THREADS="1")
    for k in list(env):
        if k.startswith(("DESC_DEBUG_", "DESC_SHARD_")):
            env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def _family(layout, T):
    """The kernel family desc_pgd_kernel_name reports: the one the layout runs a constant step with."""
    if layout == "auto":
        # the library's own choice: the small sweep up to 64 cycles; above, k_sweep_node below 2 M cycles (T = 65: ~16 k edges x 65), the
        # band sweep from there up to 256 cycles per segment (T = 256: ~52 k edges x 256), the gather layout beyond
        layout = "small" if T <= 64 else "node" if T == 65 else "band" if T <= 256 else "gather"
    if layout == "gather":
        return "k_sweep<" if T <= 64 else "k_sweep_big<"
    return {"small": "k_sweep_small<", "node": "k_sweep_node<"}.get(layout, "k_sweep_band<")


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_dispatch_launches_the_tables_instance(case):
    layout, T, step, world, name = case
    got = _dispatched()[_case_id(case)]
    assert got["last"] == name
    assert got["kernel"].startswith(_family(layout, T)), got
    if step != "adam":
        # the prefix is the constant-step instance up to its step argument
        assert name.startswith(got["kernel"]), got

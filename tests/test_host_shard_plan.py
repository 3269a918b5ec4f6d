"""Shard plan of the multi-GPU band sweep on the host side, without a GPU: the library built against the mock HIP runtime
(tests/hipmock, 256 compute units as on the MI355X; kernels do not run, device blocks read back as zeros).

Every exchange part's band sweep launches band_grid (= compute units) workgroups plus its tail pieces, and each writes one pair of
partials into the part's share of the SHARD_PARTS (1024) pairs behind the rank's S in the all-gather slice.  From 5 parts on, a
share is smaller than 256 pairs: the parts would overwrite each other's partials and the last one would write past the slice.
DESC_SHARD_PARTS is therefore clamped to SHARD_PARTS / compute units (4 here), and desc_pgd_shard_bind refuses any plan whose
part overflows its share."""
import functools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS = (2, 3, 8)
PARTS = tuple(range(1, 9))
SHARD_PARTS, MOCK_CUS = 1024, 256

CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
from desc_amd import _lib as lib
from tests.helpers import make_problem
assert hasattr(lib.load(), "hipmock_launch_count"), "must run against the mock build"
worlds, parts = json.loads(sys.argv[2]), json.loads(sys.argv[3])
mo, nn, ii, jj, rij = make_problem("uniform", n=150, p=0.6, q=0.2, sigma=0.1, seed=8)
prob = lib.ProblemArrays(nn, ii, jj, rij)
st = lib.Structure.build(prob, 30, 3, lib.BUILD_HOST, 0)
out = {}
for parts_env in parts:
    os.environ["DESC_SHARD_PARTS"] = str(parts_env)
    for world in worlds:
        got = []
        for rank in range(world):
            try:
                s = lib.Solver(prob, st, 0, rank, world)
            except Exception as e:                   # noqa: BLE001
                got.append("create: " + str(e)); continue
            try:
                info = s.shard_info()
                s.shard_bind(None, None, None)
                got.append(dict(xparts=info.xparts, slice_len=info.slice_len, segs=int(info.seg_hi - info.seg_lo), kernel=s.kernel_name()))
            except Exception as e:                   # noqa: BLE001
                got.append("bind: " + str(e))
            finally:
                s.destroy()
        out["%d/%d" % (parts_env, world)] = got
st.free()
print("RESULT " + json.dumps(out))
"""


@functools.lru_cache(maxsize=None)
def _plans():
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipmock"))
    import build_host
    so = build_host.build(ROOT, "none")
    env = dict(os.environ, DESC_AMD_LIB=so, DESC_CACHE_MB="0", DESC_DEBUG_VARIANT="3", DESC_DEBUG_ROW_CAP="560", OPENBLAS_NUM_THREADS="1")
    env.pop("DESC_SHARD_PARTS", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(WORLDS), json.dumps(PARTS)], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.parametrize("parts", PARTS)
def test_shard_parts_fit_the_partials_area(parts):
    """DESC_SHARD_PARTS = 1..8, world 2, 3 and 8, band sweep forced on a graph of ~24 bands: every rank's shard is created and bound
    (library-owned exchange buffers), and the number of exchange parts is the one asked for, clamped to SHARD_PARTS / compute units."""
    want = min(parts, SHARD_PARTS // MOCK_CUS)
    plans = _plans()
    for world in WORLDS:
        got = plans["%d/%d" % (parts, world)]
        assert len(got) == world
        for rank, g in enumerate(got):
            assert isinstance(g, dict), (parts, world, rank, g)
            assert "band" in g["kernel"], g
            assert g["xparts"] == want, (parts, world, rank, g)
        assert sum(1 for g in got if g["segs"] > 0) >= 2          # the plan is really cut between ranks
        assert len({g["slice_len"] for g in got}) == 1

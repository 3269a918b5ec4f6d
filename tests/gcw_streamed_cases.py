"""TEST INFRASTRUCTURE -- the problems of the streamed eigen-solve's tests (tests/test_gcw_streamed_host.py,
tests/test_gpu_gcw_streamed.py), built once per process.

Above the LDS kernel's cap, all Uniform_Topology(n, p, 0.2, 0.1, "uniform", seed) with S = graph_shapes.noisy_truth(mo, s); all
connected.  Gaps computed on the CPU (GCW gap lambda_3 - lambda_4 of gcw_batch_cases.gcw_gap / unit-weight spectral gap over the
spectral radius, spectral_gap below):
    U279  (279, 25/278, seed 81), S seed 181   m =  3453   0.162 / 0.53     one node past the LDS cap
    U400  (400, 0.5,    seed 82), S seed 182   m = 39915   0.610 / 0.85     long rows
    U748  (748, 12/747, seed 109), S seed 183  m =  4496   0.052 / 0.34     the refinement's cap graph
    U1112 (1112, 12/1111, seed 110), S seed 184 m =  6683   0.054 / 0.34     the streamed kernel's own cap: the whole 160 KiB of LDS
The composites' inputs: Uniform_Topology(100, 0.5, seed 91) and Uniform_Topology(300, 0.2, seed 92), gaps with S = noisy_truth (seeds
191, 192) 0.327 / 0.73 and 0.349 / 0.70 (the composites form their own S on the GPU; these say the graphs themselves are well conditioned).
tests/test_gcw_streamed_host.py asserts every one of these gaps to be at least 1e-2: no case is left out for conditioning."""
import numpy as np

from desc_amd.models import Uniform_Topology
from tests import graph_shapes as gs
from tests.gcw_batch_cases import _once

BIG = dict(U279=(279, 25.0 / 278, 81, 181, 3453), U400=(400, 0.5, 82, 182, 39915), U748=(748, 12.0 / 747, 109, 183, 4496),
           U1112=(1112, 12.0 / 1111, 110, 184, 6683))
COMPOSITE = ((100, 0.5, 91, 191), (300, 0.2, 92, 192))


def big(name):
    """(mo, S) of U279 / U400 / U748 / U1112."""
    def make():
        n, p, seed, s_seed, m = BIG[name]
        mo = Uniform_Topology(n, p, 0.2, 0.1, "uniform", seed=seed)
        assert int(mo.Ind.max()) == n and mo.Ind.shape[0] == m, (name, int(mo.Ind.max()), mo.Ind.shape[0])
        assert (gs.bfs_levels(mo.Ind, root=1) >= 0).all(), name
        return mo, gs.noisy_truth(mo, s_seed)
    return _once(("streamed_big", name), make)


def composite_models():
    """The two problems of the composite tests: one for each kernel of eig="auto"."""
    def make():
        mos = [Uniform_Topology(n, p, 0.2, 0.1, "uniform", seed=s) for n, p, s, _ in COMPOSITE]
        assert [int(mo.Ind.max()) for mo in mos] == [100, 300]
        for mo in mos:
            assert (gs.bfs_levels(mo.Ind, root=1) >= 0).all()
        return mos
    return _once("streamed_composite", make)


def composite_S():
    return _once("streamed_composite_S", lambda: [gs.noisy_truth(mo, c[3]) for mo, c in zip(composite_models(), COMPOSITE)])


def spectral_gap(mo):
    """(lambda_3 - lambda_4) / max |lambda| of the unit-weight block connection matrix (the operator of Spectral; dense)."""
    from oracle.spectral_oracle import _blk
    Ind = np.asarray(mo.Ind)
    lam = np.linalg.eigvalsh(_blk(Ind, mo.RijMat, int(Ind.max())))
    return float((lam[-3] - lam[-4]) / np.abs(lam).max())

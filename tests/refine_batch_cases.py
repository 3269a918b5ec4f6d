"""TEST INFRASTRUCTURE -- the problems and inputs of the batched refinement's tests (tests/test_refine_batch_host.py,
tests/test_gpu_refine_batch.py), built once per process.

The ten problems are the smallest shapes at which the kernel can go wrong: fewer rows than lanes (n = 8, 10, 12), rows shorter and longer
than the 16 slots a row's lanes take per round, n = 278 just above 256 (the second chunk of the score and the second round of the dot
products), a bridge (two edges carry everything between the halves) and a hub row (29 slots next to rows of 2-5).

Inputs.  S = clip(ErrVec + 0.1 N(0, 1), 2e-3, 1) and R_init = the plain spectral solution: far enough from the fixed point that the
loop really runs.  On the CPU desc_refine_oracle takes 23, 30, 14, 11, 9, 18, 9, 29, 21 and 12 iterations for k = 0 .. 9, and the same
count with the threshold moved by +-0.1 %: no case sits on the stop rule.  (With noisy_truth and a GCW start the loop stops after one
step on the larger graphs and tests nothing.)"""
import numpy as np

from desc_amd.models import Uniform_Topology
from tests import gcw_batch_cases
from tests import graph_shapes as gs

_cache = {}
ORACLE_ITERS = (23, 30, 14, 11, 9, 18, 9, 29, 21, 12)


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def models():
    """mixed_models(278) of the eigen-solve's tests (n = 8, 12, 40, 90, 150, 278, band(10, 2)), a bridged pair, a hub, n = 100."""
    def make():
        mos = list(gcw_batch_cases.mixed_models(278))
        mos += [gs.bridged(20, 16, 0.5, 0.6, 2, seed=51), gs.hub(30, 0.1, [7], seed=52), Uniform_Topology(100, 0.5, 0.3, 0.1, "uniform", seed=53)]
        assert [int(mo.Ind.max()) for mo in mos] == [8, 12, 40, 90, 150, 278, 10, 36, 30, 100]
        return mos
    return _once("models", make)


def noisy_S(mo, seed):
    m = mo.Ind.shape[0]
    return np.clip(np.asarray(mo.ErrVec, dtype=np.float64).reshape(-1) + 0.1 * np.random.default_rng(seed).standard_normal(m), 2e-3, 1.0)


def inputs():
    """(S_list, R_init_list) of the ten problems."""
    def make():
        from oracle.spectral_oracle import spectral_oracle
        mos = models()
        return [noisy_S(mo, 300 + k) for k, mo in enumerate(mos)], [spectral_oracle(mo.Ind, mo.RijMat) for mo in mos]
    return _once("inputs", make)


def oracle_results():
    """desc_refine_oracle on the ten problems: a list of (R_ref, iters_ref, score_ref).  About 7 s, computed once and left unchanged."""
    def make():
        from oracle.refine_oracle import desc_refine_oracle
        S, R0 = inputs()
        return [desc_refine_oracle(mo.Ind, mo.RijMat, s, r) for mo, s, r in zip(models(), S, R0)]
    return _once("oracle", make)


def _rotvec(v):
    """exp map of the rows of v (k x 3) -> k x 3 x 3."""
    th = np.linalg.norm(v, axis=1)
    k = v / th[:, None]
    K = np.zeros((v.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3) + np.sin(th)[:, None, None] * K + (1 - np.cos(th))[:, None, None] * (K @ K)


def dense_case():
    """The selection and the edge loops at their largest: Uniform_Topology(278, 0.9, 0.2, 0.1, seed=54), about 34.7 k edges.  S as above
    with default_rng(354); R_init = the ground truth turned by 0.05 rad about a random axis on every node.  No dense oracle."""
    def make():
        mo = Uniform_Topology(278, 0.9, 0.2, 0.1, "uniform", seed=54)
        n = int(mo.Ind.max())
        rng = np.random.default_rng(354)
        S = np.clip(np.asarray(mo.ErrVec, dtype=np.float64).reshape(-1) + 0.1 * rng.standard_normal(mo.Ind.shape[0]), 2e-3, 1.0)
        ax = rng.standard_normal((n, 3))
        ax *= 0.05 / np.linalg.norm(ax, axis=1)[:, None]
        Rg = np.transpose(np.asarray(mo.R_orig), (2, 0, 1))
        R0 = np.asfortranarray(np.transpose(Rg @ _rotvec(ax), (1, 2, 0)))
        return mo, S, R0
    return _once("dense", make)


def many_small(count=300):
    """count copies of the n = 12 problem (entry 1 of models()) with its inputs."""
    mo = models()[1]
    S, R0 = inputs()
    return [mo] * count, [S[1]] * count, [R0[1]] * count

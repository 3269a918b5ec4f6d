"""TEST INFRASTRUCTURE -- the problems and parameters of the batched MPLS tests (tests/test_mpls_batch_host.py,
tests/test_gpu_mpls_batch.py), built once per process.

The ten problems are refine_batch_cases.models(): n = 8, 12, 40, 90, 150, 278, 10 (band), 36 (bridged), 30 (hub), 100 -- the smallest
shapes at which the per-workgroup core can go wrong (fewer rows than lanes, rows shorter and longer than the 16 slots a row's lanes take
per round, n = 278 just above 256, a bridge, a hub row).  Parameters: Demo/compare_algorithms.m:26-36 with nsample = 20, problem k
sampled with seed 100 + k.

On the CPU tests/mpls_oracle.py takes ORACLE_ITERS iterations on them, and the same counts with stop_threshold moved by +-0.1 %: no
case sits on the stop rule.  The bridged problem has 2 edges without a 3-cycle and the sparse n = 278 problem 345 (the 2/3 rule of
MPLS.m:239); all ten are connected.  An entry-wise 1e-11 perturbation of RijMat (the tree held fixed) moves the oracle's R_est by at
most 6e-7, an amplification of 6e4: round-off of 1e-15 stays three orders below the 1e-7 the oracle comparison allows, and no case
sits on a quantile tie that would flip a weight.

A second set covers the sample-count classes of cemp_edge_round: problems 0, 2 and 7 with nsample = 70 (second lane group) and 300
(the two-pass class).  They are compared with the single call only: at nsample = 70 problems 2 and 7 finish within 0.1 % of the stop
threshold, which a bit-for-bit comparison does not mind and an oracle comparison would."""
import numpy as np

from tests import refine_batch_cases

_cache = {}
ORACLE_ITERS = (43, 68, 12, 8, 8, 29, 34, 49, 51, 8)
SEEDS = tuple(100 + k for k in range(10))
CLASS_PROBLEMS = (0, 2, 7)
CLASS_NSAMPLE = (70, 300)


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def models():
    return refine_batch_cases.models()


def demo_params(nsample=20, **mpls_over):
    """Demo/compare_algorithms.m:26-36 -> (CEMP_parameters without a seed, MPLS_parameters)."""
    cemp = dict(max_iter=6, reweighting=[2.0 ** k for k in range(6)], nsample=nsample)
    mpls = dict(stop_threshold=1e-3, max_iter=100, reweighting=cemp["reweighting"][-1], thresholding=[0.95, 0.9, 0.85, 0.8],
                cycle_info_ratio=1.0 / (np.arange(1, 101) + 1))
    mpls.update(mpls_over)
    return cemp, mpls


def oracle_result(k, svec_for_tree):
    """mpls_oracle on problem k with the tree built from ``svec_for_tree`` (the device's SVec).  Computed once per process and left
    unchanged; the ten take about as long as the refinement's oracle."""
    def make():
        from tests.mpls_oracle import mpls_oracle
        mo = models()[k]
        cemp, mpls = demo_params()
        return mpls_oracle(mo.Ind, mo.RijMat, cemp, mpls, seed=SEEDS[k], svec_for_tree=svec_for_tree)
    return _once(("oracle", k), make)


def many_small(count=300):
    """count copies of the n = 12 problem (entry 1 of models()) and of its seed."""
    return [models()[1]] * count, [SEEDS[1]] * count

"""Inputs and comparison helpers of tests/test_gpu_list_create.py: the two batches at the edges of k_batch_eprob and k_batch_sgn, their
synthetic inputs, the dense reference of the eigen-solve (computed once and left unchanged), and what "the same in every bit" means for
the result records of the batched families."""
import numpy as np

from tests import graph_shapes as gs

GCW_KEYS = ("iters", "products", "residual", "eigenvalues", "converged")
LAA_KEYS = ("iters", "score", "cg_iters", "cg_unconverged", "cg_residual")              # the refinement; the MPLS loop adds m_pos
IRLS_KEYS = ("l1_iters", "irls_iters", "l1_score", "irls_score", "pd_steps", "pd_ill", "pd_stuck", "pd_solves", "cg_iters_l1", "cg_iters_irls",
             "cg_unconverged", "cg_residual", "warned_edges", "comp_nodes", "comp_edges")
_cache = {}


def batches():
    """name -> the problems of a batch: graph_shapes' bands (connected, every edge on a triangle), wide enough that the eigen-solve's
    operator keeps lambda_3 - lambda_4 >= 1e-3 -- a band of width 2 on 129 or 257 nodes has 2e-5, and the batched eigen-solve then
    stops at its 500 iterations with a residual of 1e-11 instead of converging."""
    if "eprob" not in _cache:
        tri = gs.band(3, 2, seed=41)
        _cache["eprob"] = [gs.band(31, 10, seed=42, chords=[(1, 15)]), tri, gs.band(31, 10, seed=43, chords=[(1, 15), (1, 16)])]      # m = 256, 3, 257
        _cache["sgn"] = [gs.band(257, 24, seed=44), tri]                                                # n = 257, 3
    return {k: _cache[k] for k in ("eprob", "sgn")}


def inputs(mos):
    """Per problem: a synthetic S_vec and a start for the refinement (the ground truth's rotations)."""
    return [gs.noisy_truth(mo, 50 + b) for b, mo in enumerate(mos)], [np.asfortranarray(mo.R_orig) for mo in mos]


def gcw_reference(name):
    """Per problem of a batch: (the dense LAPACK GCW of oracle/spectral_oracle.py on the test's S_vec, lambda_3 - lambda_4 of its operator)."""
    if ("gcw", name) not in _cache:
        from oracle.spectral_oracle import gcw_oracle
        from tests.gcw_batch_cases import gcw_gap
        mos = batches()[name]
        _cache["gcw", name] = [(gcw_oracle(mo.Ind, mo.RijMat, s), gcw_gap(mo, s)) for mo, s in zip(mos, inputs(mos)[0])]
    return _cache["gcw", name]


def aligned_diff(R, R_ref):
    from oracle.spectral_oracle import rotation_alignment
    return float(np.abs(rotation_alignment(R, R_ref)[0] - R_ref).max())


def off_rotation(R):
    Rm = np.transpose(R, (2, 0, 1))
    return max(float(np.abs(Rm @ np.transpose(Rm, (0, 2, 1)) - np.eye(3)).max()), float(np.abs(np.linalg.det(Rm) - 1).max()))


def same(a, b):
    """Two results are the same in every bit; timings (``ms_*``, ``timings``) are not results."""
    if isinstance(a, dict):
        keys = [k for k in a if k != "timings" and not k.startswith("ms_")]
        return set(keys) == {k for k in b if k != "timings" and not k.startswith("ms_")} and all(same(a[k], b[k]) for k in keys)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))

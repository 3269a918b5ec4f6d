"""Synthetic SO(3) synchronisation problems with the distributions of the
reference's ``Models/Uniform_Topology.m`` and ``Models/Nonuniform_Topology.m``.

MATLAB's RNG streams cannot be matched, so these are *seeded re-statements of the
same distributions* (NumPy ``default_rng``), not bit-copies of a MATLAB run.  The
output struct has the reference's field names (``Uniform_Topology.m:104-109``):
``Ind`` (m x 2, 1-based, i<j, sorted (1,2),(1,3),...,(2,3),...), ``RijMat``
(3 x 3 x m), ``Rij_orig``, ``R_orig`` (3 x 3 x n), ``ErrVec`` (m,), ``AdjMat``.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np


def _project_so3(Q):
    """U*diag(1,1,det(U*V'))*V' for a stack Q (...,3,3) (Uniform_Topology.m:42-44)."""
    U, _, Vt = np.linalg.svd(Q)
    d = np.linalg.det(U @ Vt)
    U = U.copy()
    U[..., :, 2] *= d[..., None]
    return U @ Vt


def _haar(rng, count):
    return _project_so3(rng.standard_normal((count, 3, 3)))


def _abs_acos_ext(x):
    out = np.empty_like(x)
    inside = np.abs(x) <= 1
    out[inside] = np.arccos(x[inside])
    out[x > 1] = np.arccosh(x[x > 1])
    out[x < -1] = np.hypot(np.pi, np.arccosh(-x[x < -1]))
    return out


def _er_graph(rng, n, p):
    """G = tril(rand(n)<p,-1); [Ind_j,Ind_i] = find(G==1)  (Uniform_Topology.m:29-34).

    Returns 1-based (Ind_i, Ind_j) with Ind_i < Ind_j sorted by (Ind_i, Ind_j),
    generated row-block-wise so n = 10^4 does not need an n x n float matrix."""
    ii, jj = [], []
    for c in range(n - 1):                      # column c of the lower triangle: rows r > c
        rows = np.flatnonzero(rng.random(n - 1 - c) < p) + c + 1
        if rows.size:
            ii.append(np.full(rows.size, c, dtype=np.int64))
            jj.append(rows.astype(np.int64))
    if not ii:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(ii) + 1, np.concatenate(jj) + 1


class _Model(SimpleNamespace):
    @property
    def AdjMat(self):
        n = self.n
        A = np.zeros((n, n))
        A[self.Ind[:, 0] - 1, self.Ind[:, 1] - 1] = 1
        return A + A.T


def _finish(n, Ind_i, Ind_j, Rm, Rij_orig, R_orig, extra=None):
    m = Ind_i.shape[0]
    # ErrVec = abs(acos((trace(Rij_orig' * RijMat) - 1)/2))/pi  (Uniform_Topology.m:94-101)
    tr = np.einsum("lrc,lrc->l", Rij_orig, Rm) if m else np.zeros(0)
    ErrVec = _abs_acos_ext((tr - 1.0) / 2.0) / np.pi
    out = _Model(n=n, Ind=np.stack([Ind_i, Ind_j], axis=1),
                 RijMat=np.asfortranarray(np.transpose(Rm, (1, 2, 0))),
                 Rij_orig=np.asfortranarray(np.transpose(Rij_orig, (1, 2, 0))),
                 R_orig=np.asfortranarray(np.transpose(R_orig, (1, 2, 0))),
                 ErrVec=ErrVec)
    if extra:
        for k, v in extra.items():
            setattr(out, k, v)
    return out


def Uniform_Topology(n, p, q, sigma, model="uniform", seed=0):
    """Reference: Models/Uniform_Topology.m:24-110.

    ``model``: 'uniform' or 'self-consistent'.  As in the reference (``:76,83``) any
    string other than 'uniform' selects the self-consistent branch."""
    rng = np.random.default_rng(seed)
    Ind_i, Ind_j = _er_graph(rng, n, p)
    m = Ind_i.shape[0]
    R_orig = _haar(rng, n)                                           # :40-45
    Rij_orig = R_orig[Ind_i - 1] @ np.transpose(R_orig[Ind_j - 1], (0, 2, 1))   # :48-51
    Rm = Rij_orig.copy()
    noiseIndLog = rng.random(m) >= q                                 # :53
    noiseInd = np.flatnonzero(noiseIndLog)
    corrInd = np.flatnonzero(~noiseIndLog)
    if noiseInd.size:
        Rm[noiseInd] = _project_so3(Rm[noiseInd] + sigma * rng.standard_normal((noiseInd.size, 3, 3)))  # :58-65
    R_corr = _haar(rng, n)                                           # :69-74
    if corrInd.size:
        if model == "uniform":                                       # :76-82
            Rm[corrInd] = _haar(rng, corrInd.size)
        else:                                                        # :84-90
            Q = R_corr[Ind_i[corrInd] - 1] @ np.transpose(R_corr[Ind_j[corrInd] - 1], (0, 2, 1)) \
                + sigma * rng.standard_normal((corrInd.size, 3, 3))
            Rm[corrInd] = _project_so3(Q)
    return _finish(n, Ind_i, Ind_j, Rm, Rij_orig, R_orig, dict(corrupted=~noiseIndLog))


def Nonuniform_Topology(n, p, p_node_crpt, p_edge_crpt, sigma_in, sigma_out, crpt_type="uniform", seed=0):
    """Reference: Models/Nonuniform_Topology.m:26-156 ('uniform' | 'self-consistent' | 'adv')."""
    rng = np.random.default_rng(seed)
    Ind_i, Ind_j = _er_graph(rng, n, p)
    m = Ind_i.shape[0]
    R_orig = _haar(rng, n)
    Rij_orig = R_orig[Ind_i - 1] @ np.transpose(R_orig[Ind_j - 1], (0, 2, 1))
    Rm = Rij_orig.copy()
    node_crpt = rng.permutation(n)[: int(np.floor(n * p_node_crpt))] + 1       # :60-62
    crptInd = np.zeros(m, dtype=bool)
    R_crpt = _haar(rng, n)                                                     # :66-71
    # incident edge lists: Ind_full(Ind_full(:,1)==i, 2) lists first the neighbours j with
    # (j,i) = (Ind_j,Ind_i) rows i.e. smaller neighbours, then the larger ones (:37,77)
    order_lo = np.argsort(Ind_j, kind="stable")
    lo_ptr = np.searchsorted(Ind_j[order_lo], np.arange(1, n + 2))
    hi_ptr = np.searchsorted(Ind_i, np.arange(1, n + 2))
    for i in node_crpt:                                                        # :76-118
        e_lo = order_lo[lo_ptr[i - 1]:lo_ptr[i]]          # edges (x, i), x < i   -> IndMat(i,x) = -k
        e_hi = np.arange(hi_ptr[i - 1], hi_ptr[i])        # edges (i, x), x > i   -> IndMat(i,x) = +k
        cand_e = np.concatenate([e_lo, e_hi])
        cand_sign = np.concatenate([-np.ones(e_lo.size), np.ones(e_hi.size)])
        perm = rng.permutation(cand_e.size)[: int(np.floor(p_edge_crpt * cand_e.size))]   # :79-81
        for t in perm:                                                         # :84-116
            k = cand_e[t]; pos = cand_sign[t] > 0
            jn = (Ind_j[k] if pos else Ind_i[k])
            crptInd[k] = True
            R0 = _haar(rng, 1)[0]
            if crpt_type == "uniform":
                M = R0
            elif crpt_type == "self-consistent":
                M = R_crpt[i - 1] @ R_crpt[jn - 1].T
            elif crpt_type == "adv":
                M = R_crpt[i - 1] @ R_orig[jn - 1].T
            else:
                continue
            Rm[k] = M if pos else M.T
    noise = ~crptInd                                                           # :121-127
    Rm[noise] = Rm[noise] + sigma_in * rng.standard_normal((int(noise.sum()), 3, 3))
    Rm[crptInd] = Rm[crptInd] + sigma_out * rng.standard_normal((int(crptInd.sum()), 3, 3))
    if m:
        Rm = _project_so3(Rm)                                                  # :133-137
    return _finish(n, Ind_i, Ind_j, Rm, Rij_orig, R_orig, dict(corrupted=crptInd))


# ---- the batched generators: B problems drawn on the GPU in one pass (desc_models_batch_*, csrc/models_batch.hip) -------------------
# A third seeded restatement of the same distributions, defined in include/desc_amd.h: counter-based keys on (seed, stream, id,
# component).  For the same seed it does NOT produce the draws of the NumPy generators above.
_CRPT_MODES = {"uniform": 0, "self-consistent": 1, "adv": 2}


def _per_problem(name, value, B):
    """A scalar or a sequence of B values -> a list of B values."""
    if isinstance(value, str) or np.ndim(value) == 0:
        return [value] * B
    seq = list(value)
    if len(seq) != B:
        raise ValueError(f"{name} must be a scalar or hold one entry per problem ({B}), not {len(seq)}")
    return seq


def _batch_seeds(seeds):
    if seeds is None or isinstance(seeds, str) or np.ndim(seeds) != 1:
        raise ValueError("seeds must be a sequence of integers, one per problem")
    out = []
    for b, s in enumerate(seeds):
        if not isinstance(s, (int, np.integer)) or isinstance(s, bool) or not 0 <= int(s) < 2 ** 64:
            raise ValueError(f"problem {b}: the seed must be an integer in [0, 2^64)")
        out.append(int(s))
    return out


def _check_probability(b, name, x):
    x = float(x)
    if not (np.isfinite(x) and 0.0 <= x <= 1.0):
        raise ValueError(f"problem {b}: {name} must be a probability in [0, 1]")
    return x


def _check_sigma(b, name, x):
    x = float(x)
    if not (np.isfinite(x) and x >= 0.0):
        raise ValueError(f"problem {b}: {name} must be finite and >= 0")
    return x


def _check_n(b, n, cap):
    if not isinstance(n, (int, np.integer)) or isinstance(n, bool):
        raise ValueError(f"problem {b}: n must be an integer")
    n = int(n)
    if n < 2:
        raise ValueError(f"problem {b}: n = {n}, need n >= 2")
    if n > cap:
        raise ValueError(f"problem {b}: n = {n} exceeds {cap}")
    return n


def _check_totals(specs):
    """The batch-wide refusals of desc_models_batch_create."""
    N, expected = 0, 0.0
    for b, s in enumerate(specs):
        N += s.n
        expected += s.p * (0.5 * float(s.n) * float(s.n - 1))
        if N >= 2 ** 31:
            raise ValueError(f"the batch holds 2^31 nodes or more at problem {b}: split the batch")
        if expected >= float(2 ** 30):
            raise ValueError(f"the batch is expected to draw 2^30 edges or more at problem {b} (152 bytes each): split the batch")


def _draw_batch(specs, device, return_info, resident=False):
    from . import _lib
    _check_totals(specs)
    if not isinstance(device, (int, np.integer)) or isinstance(device, bool) or device < 0:
        raise ValueError("device must be a non-negative integer")
    if resident:                                     # the problems stay on the device: no rotation is copied back
        from .algorithms import ProblemBatch
        pset, timings = ProblemBatch._from_models(specs, int(device))
        return (pset, timings) if return_info else pset
    if not specs:                                    # the empty batch touches no device
        timings = {name: 0.0 for name, _ in _lib.ModelsBatchTimings._fields_}
        return ([], timings) if return_info else []
    batch = _lib.ModelsBatch(specs, device=int(device))
    try:
        arrays, timings = batch.fetch()
    finally:
        batch.destroy()
    models = []
    for b, s in enumerate(specs):
        e0, e1 = int(batch.edge_off[b]), int(batch.edge_off[b + 1])
        v0, v1 = int(batch.node_off[b]), int(batch.node_off[b + 1])
        m = e1 - e0
        Ind = np.stack([arrays["ind_i"][e0:e1].astype(np.int64) + 1, arrays["ind_j"][e0:e1].astype(np.int64) + 1], axis=1)
        models.append(_Model(n=s.n, Ind=Ind,
                             RijMat=arrays["rij"][9 * e0:9 * e1].reshape((3, 3, m), order="F"),
                             Rij_orig=arrays["rij_orig"][9 * e0:9 * e1].reshape((3, 3, m), order="F"),
                             R_orig=arrays["r_orig"][9 * v0:9 * v1].reshape((3, 3, s.n), order="F"),
                             ErrVec=arrays["err_vec"][e0:e1], corrupted=arrays["corrupted"][e0:e1].astype(bool), seed=int(s.seed)))
    return (models, timings) if return_info else models


def Uniform_Topology_batch(n, p, q, sigma, model="uniform", *, seeds, device=0, return_info=False, resident=False):
    """B = len(seeds) problems of Models/Uniform_Topology.m:24-101 drawn on the GPU in one pass.

    ``seeds``: a sequence of B integers; every other argument a scalar or a sequence of B values.  ``model``: 'uniform', any other
    string the self-consistent branch (as ``Uniform_Topology``).  Returns a list of B models with the fields and layouts of
    ``Uniform_Topology`` plus ``seed``; every ``*_batch`` solver takes them unchanged.  Problem b depends on its own arguments and seed
    only.  The draws are those of the definition in include/desc_amd.h, not the NumPy generator's for the same seed.  With
    ``return_info`` the call returns ``(models, timings)``: ms_graph, ms_nodes, ms_edges, ms_copy, ms_total.

    ``resident=True`` returns a ``ProblemBatch`` in place of the list: the same B models as its items, the problems already on the
    device for every ``*_batch`` call (desc_problem_batch_from_models).  ``n``, ``seed``, ``Ind``, ``ErrVec``, ``R_orig`` and
    ``corrupted`` are fetched once; ``RijMat``, ``Rij_orig`` and ``AdjMat`` on first access.  A problem that drew no edge is refused
    (ValueError naming it)."""
    from . import _lib
    seeds = _batch_seeds(seeds)
    B = len(seeds)
    cols = [_per_problem(name, v, B) for name, v in (("n", n), ("p", p), ("q", q), ("sigma", sigma), ("model", model))]
    cap = _lib.models_batch_max_n()
    specs = []
    for b, (nb, pb, qb, sb, mb) in enumerate(zip(*cols)):
        if not isinstance(mb, str):
            raise ValueError(f"problem {b}: model must be a string")
        specs.append(_lib.ModelSpec(kind=_lib.MODELS_KIND_UNIFORM, n=_check_n(b, nb, cap), p=_check_probability(b, "p", pb),
                                    q=_check_probability(b, "q", qb), sigma=_check_sigma(b, "sigma", sb),
                                    mode=_lib.MODELS_UNIFORM if mb == "uniform" else _lib.MODELS_SELF_CONSISTENT, seed=seeds[b]))
    return _draw_batch(specs, device, return_info, resident)


def Nonuniform_Topology_batch(n, p, p_node_crpt, p_edge_crpt, sigma_in, sigma_out, crpt_type="uniform", *, seeds, device=0,
                              return_info=False, resident=False):
    """B = len(seeds) problems of Models/Nonuniform_Topology.m:26-147 drawn on the GPU in one pass; arguments and result as
    ``Uniform_Topology_batch`` (``resident`` included).  ``crpt_type``: 'uniform' | 'self-consistent' | 'adv'.  The two ``randperm``s are keyed selections: the
    corrupted nodes are the floor(n p_node_crpt) nodes with the smallest node keys, node i corrupts the floor(p_edge_crpt deg_i)
    incident edges with the smallest (i, edge) keys, and an edge both endpoints selected belongs to the endpoint with the larger
    node key."""
    from . import _lib
    seeds = _batch_seeds(seeds)
    B = len(seeds)
    cols = [_per_problem(name, v, B) for name, v in (("n", n), ("p", p), ("p_node_crpt", p_node_crpt), ("p_edge_crpt", p_edge_crpt),
                                                     ("sigma_in", sigma_in), ("sigma_out", sigma_out), ("crpt_type", crpt_type))]
    cap = _lib.models_batch_max_n()
    specs = []
    for b, (nb, pb, pn, pe, si, so, ct) in enumerate(zip(*cols)):
        if not isinstance(ct, str) or ct not in _CRPT_MODES:
            raise ValueError(f"problem {b}: unknown crpt_type {ct!r} (uniform | self-consistent | adv)")
        specs.append(_lib.ModelSpec(kind=_lib.MODELS_KIND_NONUNIFORM, n=_check_n(b, nb, cap), p=_check_probability(b, "p", pb),
                                    p_node_crpt=_check_probability(b, "p_node_crpt", pn),
                                    p_edge_crpt=_check_probability(b, "p_edge_crpt", pe), sigma_in=_check_sigma(b, "sigma_in", si),
                                    sigma_out=_check_sigma(b, "sigma_out", so), mode=_CRPT_MODES[ct], seed=seeds[b]))
    return _draw_batch(specs, device, return_info, resident)

"""Host-side mirror of the reference's solver entry points.

The reference is MATLAB and no MATLAB/Octave/MEX toolchain exists in the build
environment, so the host layer above the C ABI is written in Python with the
reference's names, argument meaning and conventions:

    S_vec = DESC_PGD(Ind, RijMat, params)        Algorithms/DESC_PGD.m:14

``Ind`` is ``m x 2`` with 1-based node ids ``i<j``; ``RijMat`` is ``3 x 3 x m``;
``params`` is a struct-like object (attributes or dict keys) with the fields the
reference reads: ``iters`` (:170), ``Gradient`` (:207), ``make_plots`` (:235) and,
when plotting, ``ErrVec`` / ``R_orig`` (:236-238).  ``learning_rate`` is accepted
and ignored, as in the reference (:169 is commented out).  Optional fields that do
not exist in the reference: ``seed`` (cycle-sampling seed; MATLAB uses its global
RNG), ``device``, ``verbose``, ``build_where``.

All numerical work of the hot path happens in libdesc_amd.so on the GPU; this file
only marshals arguments.  MATLAB wrappers with the same signatures and the MEX shim
over the same ABI are in matlab/.
"""
from __future__ import annotations

import collections.abc
import contextlib
import ctypes as C

import os

import numpy as np

from . import _lib
from .stepsize import ConstantStepSize, HybridGradient, PiecewiseStepSize


def _get(params, name, default=None):
    if isinstance(params, dict):
        return params.get(name, default)
    return getattr(params, name, default)


def _set(params, name, value):
    if isinstance(params, dict):
        params[name] = value
    else:
        try:
            setattr(params, name, value)
        except Exception:
            pass


def marshal_edges(Ind, RijMat=None):
    """MATLAB arrays -> C-ABI arrays.

    Returns (n, ind_i, ind_j, rij, perm): 0-based int32 endpoints sorted by (i,j),
    rij as an (m*9,) float64 buffer in the reference's memory order
    (element (r,c,l) at 9*l + r + 3*c), and ``perm`` such that row ``perm[t]`` of the
    caller's ``Ind`` is the t-th sorted edge (``None`` when already sorted).  The
    reference silently requires sorted input (DESC_PGD.m:5,31-34); unsorted input is
    sorted here and outputs are returned in the caller's order."""
    Ind = np.asarray(Ind)
    if Ind.ndim != 2 or Ind.shape[1] != 2:
        raise ValueError("Ind must be m x 2")
    m = Ind.shape[0]
    if Ind.dtype.kind not in "iuf":
        raise ValueError("Ind must hold integer node ids")
    try:        # one threaded pass of the library (desc_marshal_edges): checks, 0-based int32 endpoints, n = max(Ind(:)) (DESC_PGD.m:21), order
        n, ii, jj, is_sorted = _lib.marshal_edges_native(Ind)
    except _lib.DescError as e:
        if e.code != _lib.ERR_INVALID:
            raise
        raise ValueError(str(e).split(": ", 1)[-1]) from None
    perm = None
    if not is_sorted:
        perm = np.lexsort((jj, ii))
        ii, jj = ii[perm], jj[perm]
        if m > 1 and np.any((ii[1:] == ii[:-1]) & (jj[1:] == jj[:-1])):
            raise ValueError("Ind lists an edge twice")
    rij = None
    if RijMat is not None:
        R = np.asarray(RijMat, dtype=np.float64)
        if R.shape != (3, 3, m):
            raise ValueError("RijMat must be 3 x 3 x m")
        if perm is None and R.flags.f_contiguous:
            rij = R.reshape(-1, order="F")            # MATLAB memory order of a 3x3xm array, r + 3c + 9l: the ABI's own, no copy
        else:
            if any(st % 8 for st in R.strides):
                R = np.ascontiguousarray(R)
            rij = _lib.marshal_rij_native(R, perm)    # any other strides (NumPy's C order) and / or the edge permutation: one threaded pass
    return n, ii, jj, rij, perm


def gradient_to_params(G, p: _lib.Params):
    """Translate a params.Gradient plugin object into the flat C struct."""
    if isinstance(G, ConstantStepSize):
        p.step_kind = _lib.STEP_CONSTANT
        p.lr = G.learning_rate
        p.t0 = 0
    elif isinstance(G, PiecewiseStepSize):
        p.step_kind = _lib.STEP_PIECEWISE
        p.lr = G.learning_rate
        p.decay_interval = float(G.decay_interval)
        p.t0 = int(G.t)
    elif isinstance(G, HybridGradient):
        p.step_kind = _lib.STEP_HYBRID
        p.lr = G.lr
        p.beta1, p.beta2 = G.beta_1, G.beta_2
        p.decay_interval = float(G.decay_interval)
        p.hybrid_strategy = int(G.strategy)
        p.t0 = int(G.t)
    elif callable(getattr(G, "GetStep", None)):
        # any other handle object with a GetStep method (DESC_PGD.m:207): the library hands out grad_long and takes the step back
        p.step_kind = _lib.STEP_EXTERNAL
        p.t0 = 0
    else:
        raise TypeError("params.Gradient must be an object with a callable GetStep(grad_long) method (DESC_PGD.m:207): a "
                        "ConstantStepSize, PiecewiseStepSize or HybridGradient (Utils/*.m), which run inside the HIP sweep, "
                        "or any plugin of your own, which runs between the gradient pass and the apply pass")


def is_external(G):
    """True for a params.Gradient plugin the library does not know by class: its GetStep is called from the loop."""
    return not isinstance(G, (ConstantStepSize, PiecewiseStepSize, HybridGradient)) and callable(getattr(G, "GetStep", None))


def make_c_params(params):
    G = _get(params, "Gradient")
    if G is not None and is_external(G) and getattr(G, "device_tensors", False):
        _lib.torch_for_device_mode()          # torch has to come before the library is loaded
    p = _lib.default_params()
    iters = _get(params, "iters")
    if iters is None:
        raise ValueError("params.iters is required (DESC_PGD.m:170)")
    p.iters = int(iters)
    if G is None:
        raise ValueError("params.Gradient is required (DESC_PGD.m:207)")
    gradient_to_params(G, p)
    p.seed = int(_get(params, "seed", 0))
    p.device = int(_get(params, "device", 0))
    p.verbose = 1 if _get(params, "verbose", True) else 0
    p.build_where = int(_get(params, "build_where", _lib.BUILD_DEVICE))
    return p, G


def DESC_PGD(Ind, RijMat, params, return_info=False, _marshalled=None):
    """[S_vec] = DESC_PGD(Ind, RijMat, params) -- Algorithms/DESC_PGD.m:14.

    Returns the estimated corruption level of every edge (length-m vector in the
    caller's edge order).  With ``return_info`` also a dict with the objective and
    average-change traces, iteration count, timings and structure sizes.

    ``params.Gradient`` is any object with a ``GetStep(grad_long)`` method (:207).  The three classes of desc_amd.stepsize (and their
    subclasses) run inside the HIP sweep.  Any other object is called once per iteration between the gradient pass and the apply pass
    (_run_external): by default with a NumPy float64 array of m_cycle entries, returning one (2 x 8 m_cycle bytes over PCIe per
    iteration: slow, always available); with the attribute ``device_tensors = True`` with a float64 torch tensor on the solver's GPU,
    read-only, returning a tensor of the same dtype, device and length (import torch before desc_amd loads its library).
    ``grad_long`` follows the cycle order of the problem sorted by (i, j): segment l at cum_ind[l] .. cum_ind[l+1]; an unsorted ``Ind``
    permutes the edge vectors only.
    ``_marshalled`` (internal, used by DESC()): (perm, ProblemArrays, DeviceProblem or a callable that returns it) already prepared."""
    p, G = make_c_params(params)
    make_plots = bool(_get(params, "make_plots", False))
    if make_plots and (_get(params, "ErrVec") is None or _get(params, "R_orig") is None):
        raise ValueError("params.make_plots=true reads params.ErrVec and params.R_orig (DESC_PGD.m:236-238)")
    if _marshalled is None:
        n, ii, jj, rij, perm = marshal_edges(Ind, RijMat)
        if ii.shape[0] == 0:
            raise ValueError("empty edge list")
        prob = _lib.ProblemArrays(n, ii, jj, rij)
        dprob = prob
    else:
        perm, prob, dprob = _marshalled
    verbose = bool(p.verbose)
    cb = None
    if verbose:        # the reference's per-iteration line (DESC_PGD.m:241), streamed by the library while the loop runs
        def _line(user, it, avg, obj):
            print("iter %d: average change in S_vec %f, objective value: %f" % (it, avg, obj), flush=True)
        cb = _lib.PROGRESS_FN(_line)
        p.progress = C.cast(cb, C.c_void_p)
        p.verbose = 0
    hybrid_state = isinstance(G, HybridGradient) and G.strategy == 0       # carries m_cycle-long moment vectors in and out
    external = is_external(G)                                              # a plugin of the caller's: its GetStep runs between two passes
    if _marshalled is None and not make_plots and not return_info and not hybrid_state and not external:
        # the reference's own signature, S_vec = DESC_PGD(Ind, RijMat, params): ONE C call (desc_pgd_solve), in which the rotations go up
        # while the structure is built (C4: 13 ms hidden)
        if verbose:
            print("compute R cycle")                      # DESC_PGD.m:132
            print("S0Mat")                                # :145
            print("Initialization completed!")            # :160
            print("Reweighting Procedure Started ...")    # :162
        out = _lib.solve(prob, p)
        if isinstance(G, (PiecewiseStepSize, HybridGradient)):
            G.t = int(out["t_end"])
        if perm is None:
            return out["S_vec"]
        S_vec = np.empty_like(out["S_vec"])
        S_vec[perm] = out["S_vec"]
        return S_vec
    try:
        st = _lib.Structure.build(prob, p.n_sample_min, p.seed, p.build_where, p.device)
    except _lib.DescError as e:
        # the device builder refuses graphs whose bitmaps / per-edge staging exceed its budget
        if p.build_where != _lib.BUILD_DEVICE or e.code != _lib.ERR_TOO_LARGE:
            raise
        st = _lib.Structure.build(prob, p.n_sample_min, p.seed, _lib.BUILD_HOST, p.device)
    try:
        sizes = st.sizes()                    # O(1): the structure stays on the device
        ms_structure = sizes.pop("ms_build")
        if callable(dprob):
            dprob = dprob()                       # DESC(): the device problem has been going up on a helper thread meanwhile
        solver = _lib.Solver(dprob, st, p.device)
    finally:
        st.free()
    try:
        if verbose:
            print("compute R cycle")                      # DESC_PGD.m:132
            print("S0Mat")                                # :145
            print("Initialization completed!")            # :160
            print("Reweighting Procedure Started ...")    # :162
        adam = None
        if isinstance(G, HybridGradient) and G.strategy == 0:
            mt = G.m_t if (G.t > 0 and G.m_t is not None) else np.zeros(solver.m_cycle)
            vt = G.v_t if (G.t > 0 and G.v_t is not None) else np.zeros(solver.m_cycle)
            if mt.shape[0] != solver.m_cycle:
                raise ValueError("HybridGradient state has a different length than this problem's cycle vector")
            adam = (np.ascontiguousarray(mt, dtype=np.float64).copy(), np.ascontiguousarray(vt, dtype=np.float64).copy())
        if external:
            out = _run_external(solver, p, G, params, prob, dprob, perm, verbose, make_plots)
        elif not make_plots:
            out = solver.run(p, adam=adam)
        else:
            out = _run_with_plots(solver, p, params, prob, dprob, perm, verbose, adam)
    finally:
        solver.destroy()
    # plugin state after the run (handle-object semantics)
    if isinstance(G, (PiecewiseStepSize, HybridGradient)):
        G.t = int(out["t_end"])
    if adam is not None:
        G.m_t, G.v_t = out["adam_m"], out["adam_v"]
    S_sorted = out["S_vec"]
    if perm is not None:
        S_vec = np.empty_like(S_sorted)
        S_vec[perm] = S_sorted
    else:
        S_vec = S_sorted
    if return_info:
        info = dict(out)
        info.update(sizes)
        info["ms_structure"] = ms_structure
        return S_vec, info
    return S_vec


def _check_sequence(problems):
    import collections.abc
    if isinstance(problems, (str, bytes, np.ndarray)) or not isinstance(problems, collections.abc.Sequence):
        raise ValueError("problems must be a sequence of (Ind, RijMat) pairs or of model objects with .Ind / .RijMat")


class _Marshalled:
    """A problem of a batch call that has been through marshal_edges already (DESC_init_batch hands these to DESC_PGD_batch)."""

    def __init__(self, prob, perm):
        self.prob, self.perm = prob, perm


def _marshal_problems(problems, rotations=True):
    """The problems of a batch call -> (list of ProblemArrays, list of edge permutations); ValueError names the problem.  A ProblemBatch
    was marshalled when it was made: its host mirror comes back, with the rotations (one fetch for a generated set) unless
    ``rotations`` is False."""
    if isinstance(problems, ProblemBatch):
        return (problems._host_problems() if rotations else problems._index_problems()), problems.perms
    probs, perms = [], []
    for b, item in enumerate(problems):
        if isinstance(item, _Marshalled):
            probs.append(item.prob); perms.append(item.perm)
            continue
        if hasattr(item, "Ind") and hasattr(item, "RijMat"):
            Ind, RijMat = item.Ind, item.RijMat
        else:
            try:
                Ind, RijMat = item
            except (TypeError, ValueError):
                raise ValueError(f"problem {b}: expected an (Ind, RijMat) pair or an object with .Ind / .RijMat") from None
        try:
            n, ii, jj, rij, perm = marshal_edges(Ind, RijMat)
        except ValueError as e:
            raise ValueError(f"problem {b}: {e}") from None
        if ii.shape[0] == 0:
            raise ValueError(f"problem {b}: empty edge list")
        probs.append(_lib.ProblemArrays(n, ii, jj, rij))
        perms.append(perm)
    return probs, perms


class _SetItem:
    """Item b of a ProblemBatch made from (Ind, RijMat) pairs."""

    def __init__(self, Ind, RijMat):
        self.Ind, self.RijMat = Ind, RijMat


class _ResidentModel:
    """Item b of a generated ProblemBatch: a model whose small fields are on the host and whose RijMat / Rij_orig / AdjMat are fetched
    from the device on first access."""

    def __init__(self, owner, b, **small):
        self._owner, self._b = owner, b
        self.__dict__.update(small)

    def _blocks(self, flat):
        e0, e1 = self._owner._edge_range(self._b)
        return flat[9 * e0:9 * e1].reshape((3, 3, e1 - e0), order="F")

    @property
    def RijMat(self):
        return self._owner._host_problems()[self._b].rij.reshape((3, 3, -1), order="F")

    @property
    def Rij_orig(self):
        return self._blocks(self._owner._rij_orig())

    @property
    def AdjMat(self):
        A = np.zeros((self.n, self.n))
        A[self.Ind[:, 0] - 1, self.Ind[:, 1] - 1] = 1
        return A + A.T


class ProblemBatch(collections.abc.Sequence):
    """The problems of a study, validated, laid out and uploaded to the GPU once (desc_problem_batch_*): every ``*_batch`` call takes a
    ProblemBatch where it takes a list of problems, and gives the same bits.  Spectral_batch, GCW_batch, DESC_refine_batch,
    DESC_PGD_batch, DESC_init_batch, DESC_batch, CEMP_batch, CEMP_GCW_batch, MST_batch, CEMP_MST_batch, MPLS_batch, IRLS_GM_batch and
    IRLS_L12_batch create their handles ON the set -- no marshalling, no validation, no CSR build and no 72-byte-per-edge upload per
    call, and no rotation of a generated set comes down to the host (MST_batch fetches the 72-byte blocks of its n_b - 1 tree edges).
    linprog_sij_batch alone reads the set's host mirror (its plan is a host codegree merge) and saves the marshalling.

    ``problems`` as for DESC_PGD_batch; ``device`` the GPU the set lives on (a call whose ``device`` / ``params.device`` differs is
    refused); ``csr``: ``"host"`` builds the per-problem CSR on host threads, ``"device"`` builds the same arrays in one launch.
    A Sequence of B items with ``.Ind`` / ``.RijMat``; ``perms`` holds the edge permutations of the marshalling.  ``close()`` (or the
    end of a ``with`` block) drops the set; handles that are still running on it keep its device arrays alive.
    ``Uniform_Topology_batch(..., resident=True)`` returns a set drawn on the device; its items are models.

    Refused (ValueError): what a ``*_batch`` call refuses of its problems, a ``csr`` other than the two, a negative ``device``."""

    def __init__(self, problems, device=0, csr="host"):
        _check_sequence(problems)
        if not isinstance(csr, str) or csr not in _lib.CSR_WHERE:
            raise ValueError(f"csr must be 'host' or 'device', not {csr!r}")
        if not isinstance(device, (int, np.integer)) or isinstance(device, bool) or device < 0:
            raise ValueError("device must be a non-negative integer")
        probs, self.perms = _marshal_problems(problems)
        self._items = [it if hasattr(it, "Ind") and hasattr(it, "RijMat") else _SetItem(*it) for it in problems]
        self.device, self._gen, self._orig = int(device), None, None
        with _invalid_as_value_error():
            self._set = _lib.ProblemBatch(probs, self.device, csr)

    @classmethod
    def _from_models(cls, specs, device):
        """The set of a generator call (models._draw_batch): no rotation reaches the host.  Returns (set, the generator's timings)."""
        self = cls.__new__(cls)
        self.device, self._orig = int(device), None
        gen = _lib.ModelsBatch(specs, device=self.device)
        try:
            small, timings = gen.fetch(only=("r_orig", "err_vec", "corrupted"))
            with _invalid_as_value_error():
                self._set = _lib.ProblemBatch.from_models(gen)
        except Exception:
            gen.destroy()
            raise
        self._gen = gen                              # Rij_orig stays with the generator until somebody asks
        self.perms = [None] * len(specs)
        self._items = []
        for b, (s, q) in enumerate(zip(specs, self._set.probs)):
            e0, e1 = self._edge_range(b)
            v0, v1 = int(gen.node_off[b]), int(gen.node_off[b + 1])
            self._items.append(_ResidentModel(self, b, n=int(s.n), seed=int(s.seed),
                                              Ind=np.stack([q.ind_i.astype(np.int64) + 1, q.ind_j.astype(np.int64) + 1], axis=1),
                                              ErrVec=small["err_vec"][e0:e1], corrupted=small["corrupted"][e0:e1].astype(bool),
                                              R_orig=small["r_orig"][9 * v0:9 * v1].reshape((3, 3, int(s.n)), order="F")))
        return self, timings

    def __len__(self):
        return len(self._items)

    def __getitem__(self, b):
        return self._items[b]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def closed(self):
        return not self._set.handle

    @property
    def built_where(self):
        """``"host"`` or ``"device"``: the builder of the set's CSR."""
        return "device" if self._set.built_where == _lib.BUILD_DEVICE else "host"

    def bytes(self):
        """(bytes copied to the device, bytes copied back) by the set so far."""
        return self._set.bytes()

    def close(self):
        self._set.close()
        if self._gen is not None:
            self._gen.destroy()

    def _edge_range(self, b):
        return int(self._set.edge_off[b]), int(self._set.edge_off[b + 1])

    def _index_problems(self):
        return self._set.probs

    def _host_problems(self):
        return self._set.host_problems()

    def _rij_orig(self):
        if self._orig is None:
            if not self._gen.handle:
                raise ValueError("the ProblemBatch is closed")
            self._orig = self._gen.fetch(only=("rij_orig",))[0]["rij_orig"]
        return self._orig


def _resident(problems, device):
    """The _lib.ProblemBatch behind ``problems`` if that is a ProblemBatch, else None; the call's device must be the set's."""
    if not isinstance(problems, ProblemBatch):
        return None
    if int(device) != problems.device:
        raise ValueError(f"device = {int(device)} differs from the device of the ProblemBatch ({problems.device})")
    if problems.closed:
        raise ValueError("the ProblemBatch is closed")
    return problems._set


@contextlib.contextmanager
def _invalid_as_value_error():
    """A refusal of the library (DESC_ERR_INVALID) leaves the block as ValueError, without the entry point's name in front."""
    try:
        yield
    except _lib.DescError as e:
        if e.code == _lib.ERR_INVALID:
            raise ValueError(str(e).split(": ", 1)[-1]) from None
        raise


@contextlib.contextmanager
def _batch_handle(cls, *args, **kw):
    """``cls(*args, **kw)``, one of _lib's batched handles, for the length of a with block: what create refuses is a ValueError, and
    the handle is destroyed however the block ends."""
    with _invalid_as_value_error():
        batch = cls(*args, **kw)
    try:
        yield batch
    finally:
        batch.destroy()


_BUILD_WHERE = {"host": _lib.BUILD_HOST, "device": _lib.BUILD_DEVICE}


def _check_build(build):
    """``build`` of the batched DESC calls -> BUILD_HOST / BUILD_DEVICE."""
    if not isinstance(build, str) or build not in _BUILD_WHERE:
        raise ValueError(f"build must be 'host' or 'device', not {build!r}")
    return _BUILD_WHERE[build]


def _check_seeds(seeds, B):
    """``seeds`` as a list of B ints, or None."""
    if seeds is None:
        return None
    seeds = [int(x) for x in seeds]
    if len(seeds) != B:
        raise ValueError(f"seeds must hold one entry per problem ({B}), not {len(seeds)}")
    return seeds


def DESC_PGD_batch(problems, params, seeds=None, return_info=False, build="host", _set=None):
    """DESC_PGD on B independent problems in one GPU pass (desc_pgd_batch_*; the reference has no such call).

    ``problems`` is a sequence of ``(Ind, RijMat)`` pairs or of model objects with ``.Ind`` / ``.RijMat``; ``params`` as for DESC_PGD,
    one for the whole batch; ``seeds`` an optional sequence of per-problem sampling seeds (default: ``params.seed`` for every problem).
    Problem b gets what ``DESC_PGD(Ind_b, RijMat_b, params)`` returns with the same seed and the host structure builder: its own
    n_sample, traces, patience rule and stop iteration; its result does not depend, in any bit, on the batch around it.
    ``build``: ``"host"`` builds the cycle structures per problem on host threads; ``"device"`` builds the same index arrays, element
    for element, in five launches for the whole batch (desc_pgd_batch_create_where) -- every result bit is the same.  A batch outside
    the device builder's staging caps is built on the host without failing; ``built_where`` says which builder ran.

    Returns a list of S_vec arrays (caller's edge order).  With ``return_info`` a list of dicts: ``S_vec``, ``iters_run``, ``obj_vals``,
    ``average_change``, ``n_sample``, ``w`` (cycle order of the problem sorted by (i, j)), ``t_end``, ``built_where`` (``"host"`` or
    ``"device"``) and the call's ``timings``; with a HybridGradient (Adam) also ``m_t`` / ``v_t``.  The plugin object is shared by the batch and is NOT updated: its counter ``t`` is
    read as the starting counter of every problem, the moments start at zero, and each problem's state comes back in its dict.

    Refused (ValueError): a Gradient object of the caller's own (external GetStep), ``make_plots``, a problem whose n_sample exceeds 64
    (solve it with DESC_PGD), a ``build`` other than ``"host"`` / ``"device"``."""
    where = _check_build(build)
    _check_sequence(problems)
    G = _get(params, "Gradient")
    if G is not None and is_external(G):
        raise ValueError("DESC_PGD_batch runs the three step rules of Utils/ (ConstantStepSize, PiecewiseStepSize, HybridGradient); "
                         "a Gradient object with a GetStep of its own runs through DESC_PGD, one problem at a time")
    if bool(_get(params, "make_plots", False)):
        raise ValueError("DESC_PGD_batch does not support params.make_plots: use DESC_PGD for the traced run of one problem")
    B = len(problems)
    seeds = _check_seeds(seeds, B)
    p, G = make_c_params(params)
    p.verbose = 0
    pset = _set if _set is not None else _resident(problems, p.device)
    if B == 0:
        return []
    probs, perms = _marshal_problems(problems, rotations=pset is None)
    with _batch_handle(_lib.Batch, probs, p, seeds, where, on=pset) as batch:
        built_where = "device" if batch.built_where == _lib.BUILD_DEVICE else "host"
        hybrid = isinstance(G, HybridGradient) and G.strategy == 0
        adam = (np.zeros(max(batch.m_cycle, 1)), np.zeros(max(batch.m_cycle, 1))) if hybrid else None
        if adam is not None:
            adam = (adam[0][:batch.m_cycle], adam[1][:batch.m_cycle])
        outs, timings = batch.run(p, want_w=return_info, adam=adam)
        if batch.built_where == _lib.BUILD_DEVICE:       # device time of the builder's five launches
            timings.update({"ms_build_" + name: ms for name, ms in batch.build_laps().items()})
    result = []
    for o, perm in zip(outs, perms):
        S_vec = o["S_vec"]
        if perm is not None:
            S_sorted, S_vec = S_vec, np.empty_like(S_vec)
            S_vec[perm] = S_sorted
        if not return_info:
            result.append(S_vec)
            continue
        d = dict(S_vec=S_vec, iters_run=o["iters_run"], obj_vals=o["obj"], average_change=o["avg"], n_sample=o["n_sample"], w=o["w"],
                 t_end=o["t_end"], built_where=built_where, timings=timings)
        if hybrid:
            d["m_t"], d["v_t"] = o["adam_m"], o["adam_v"]
        result.append(d)
    return result


def _check_batch_sizes(probs, cap, what, instead):
    """A batched kernel's size cap (nodes of one problem), checked before the device is touched."""
    for b, q in enumerate(probs):
        if q.n > cap:
            raise ValueError(f"problem {b}: n = {q.n} exceeds {cap} (the {what} must fit the LDS of one workgroup): solve it with {instead}")


def _check_eig(eig):
    """``eig`` of the calls built on the batched eigen-solve: ``"lds"`` (the default: the four blocks in LDS), ``"streamed"`` (the
    blocks in global memory, one staging block in LDS) or ``"auto"`` (each problem by its own n)."""
    _lib.gcw_eig_mode(eig)
    return eig


def _check_gcw_batch_sizes(probs, eig="lds", instead="GCW / DESC_init"):
    if eig == "lds":
        _check_batch_sizes(probs, _lib.gcw_batch_max_n(), "3n x 6 blocks of the eigen-solve", instead)
    else:
        _check_batch_sizes(probs, _lib.gcw_batch_streamed_max_n(), "one 3n x 6 block of the streamed eigen-solve", instead)


def _sorted_s_list(probs, perms, S_list, noun="S_vec", ok=lambda S: np.isfinite(S) & (S >= 0),
                   describe_bad=lambda q, perm, t: f"S_vec holds a negative or non-finite entry (node {int(q.ind_i[t])})"):
    """One S_vec per problem in the caller's edge order -> the concatenation in the library's order; refusals name the problem.
    ``ok``: the entries a call takes; ``describe_bad``: its words for sorted entry t of problem q that is not among them."""
    if isinstance(S_list, (str, bytes)) or not hasattr(S_list, "__len__") or len(S_list) != len(probs):
        got = len(S_list) if hasattr(S_list, "__len__") else type(S_list).__name__
        raise ValueError(f"S_list must hold one {noun} per problem ({len(probs)}), not {got}")
    parts = []
    for b, (q, perm, S) in enumerate(zip(probs, perms, S_list)):
        S = np.asarray(S, dtype=np.float64).reshape(-1)
        if S.shape[0] != q.m:
            raise ValueError(f"problem {b}: {noun} must have one entry per edge ({q.m}), not {S.shape[0]}")
        if perm is not None:
            S = S[perm]
        bad = np.flatnonzero(~ok(S))
        if bad.size:
            raise ValueError(f"problem {b}: {describe_bad(q, perm, bad[0])}")
        parts.append(S)
    return np.concatenate(parts) if parts else np.zeros(0)


def _gcw_batch_run(probs, device, eig="lds", pset=None, **run_args):
    with _batch_handle(_lib.GcwBatch, probs, device, eig, on=pset) as batch:
        return batch.run(**run_args)


def Spectral_batch(problems, device=0, return_info=False, eig="lds"):
    """Spectral (Algorithms/Spectral.m:15) on B independent small problems in one GPU launch (desc_gcw_batch_*; the reference has no such
    call).  ``problems`` as for DESC_PGD_batch.  Returns a list of R (3 x 3 x n_b); with ``return_info`` a list of (R, info) with the
    record Spectral() gives plus the call's ``timings``.  Problem b's result does not depend, in any bit, on the batch around it.

    ``eig`` says where the kernel keeps its four 3n x 6 blocks.  ``"lds"`` (the default) keeps them in LDS and takes
    ``_lib.gcw_batch_max_n()`` (278) nodes.  ``"streamed"`` keeps them in global memory and stages the source of each product in LDS:
    ``_lib.gcw_batch_streamed_max_n()`` (1112) nodes, the same bits, slower where both apply.  ``"auto"`` solves a problem of at most 278
    nodes in LDS and a larger one streamed (at most two launches); ``info["eig"]`` says which kernel solved a problem.

    Refused (ValueError): an empty edge list, an ``eig`` other than the three, a problem of more nodes than the cap of ``eig`` (solve
    it with Spectral)."""
    _check_eig(eig)
    _check_sequence(problems)
    pset = _resident(problems, device)
    probs, perms = _marshal_problems(problems, rotations=pset is None)
    if not probs:
        return []
    _check_gcw_batch_sizes(probs, eig)
    outs, timings = _gcw_batch_run(probs, device, eig, pset, normalize_rows=False)
    return [(R, dict(info, timings=timings)) for R, info in outs] if return_info else [R for R, _ in outs]


def GCW_batch(problems, S_list, device=0, return_info=False, eig="lds"):
    """GCW (Utils/GCW.m) on B independent small problems in one GPU launch: ``S_list[b]`` is problem b's S_vec in the caller's edge
    order; the weights 1/(S^1.5 + 1e-8) are formed on the device.  Returns a list of R (3 x 3 x n_b); with ``return_info`` a list of
    (R, info).  ``eig`` as for Spectral_batch.  Refused (ValueError, before the device is touched): S_list of the wrong length or an
    entry of the wrong size, a negative or non-finite S entry, an empty edge list, an ``eig`` other than ``"lds"`` / ``"streamed"`` /
    ``"auto"``, a problem of more nodes than the cap of ``eig`` (``_lib.gcw_batch_max_n()`` by default; solve it with GCW)."""
    _check_eig(eig)
    _check_sequence(problems)
    pset = _resident(problems, device)
    probs, perms = _marshal_problems(problems, rotations=pset is None)
    S = _sorted_s_list(probs, perms, S_list)
    if not probs:
        return []
    _check_gcw_batch_sizes(probs, eig)
    outs, timings = _gcw_batch_run(probs, device, eig, pset, s_vec=S)
    return [(R, dict(info, timings=timings)) for R, info in outs] if return_info else [R for R, _ in outs]


def DESC_init_batch(problems, params, seeds=None, return_info=False, build="host", eig="lds", _set=None):
    """DESC_init (Algorithms/DESC_init.m: DESC_PGD, then GCW) on B independent small problems: DESC_PGD_batch's pass, then the batched
    eigen-solve on the resulting S_vec -- two GPU passes for the whole batch.  Returns a list of (R_est, S_vec); problem b's S_vec is
    bit for bit what DESC_PGD_batch returns for it.  With ``return_info`` a list of (R_est, S_vec, dict(pgd=..., gcw=...)).
    ``build`` is DESC_PGD_batch's (``dict["pgd"]["built_where"]`` says which builder ran); ``eig`` is Spectral_batch's.
    Refused (ValueError, before the device is touched): what DESC_PGD_batch refuses, an ``eig`` other than ``"lds"`` / ``"streamed"`` /
    ``"auto"``, and a problem of more nodes than the cap of ``eig`` (``_lib.gcw_batch_max_n()`` by default; solve it with DESC_init)."""
    _check_eig(eig)
    _check_build(build)
    _check_sequence(problems)
    G = _get(params, "Gradient")
    if G is not None and is_external(G):
        raise ValueError("DESC_init_batch runs the three step rules of Utils/ (ConstantStepSize, PiecewiseStepSize, HybridGradient); "
                         "a Gradient object with a GetStep of its own runs through DESC_init, one problem at a time")
    if bool(_get(params, "make_plots", False)):
        raise ValueError("DESC_init_batch does not support params.make_plots: use DESC_init for the traced run of one problem")
    seeds = _check_seeds(seeds, len(problems))
    pset = _set if _set is not None else _resident(problems, _get(params, "device", 0))
    probs, perms = _marshal_problems(problems, rotations=pset is None)
    _check_gcw_batch_sizes(probs, eig)
    pgd = DESC_PGD_batch([_Marshalled(q, perm) for q, perm in zip(probs, perms)], params, seeds=seeds, return_info=True, build=build,
                         _set=pset)
    if not probs:
        return []
    # DESC_PGD_batch gave S_vec in the caller's order; the eigen-solve takes the library's
    S_sorted = [d["S_vec"] if perm is None else d["S_vec"][perm] for d, perm in zip(pgd, perms)]
    outs, timings = _gcw_batch_run(probs, int(_get(params, "device", 0)), eig, pset, s_vec=np.concatenate(S_sorted))
    if return_info:
        return [(R, d["S_vec"], dict(pgd=d, gcw=dict(info, timings=timings))) for (R, info), d in zip(outs, pgd)]
    return [(R, d["S_vec"]) for (R, _), d in zip(outs, pgd)]


def _check_refine_batch_sizes(probs):
    _check_batch_sizes(probs, _lib.refine_batch_max_n(), "per-node state of the refinement", "DESC")


def _r_init_list(probs, R_init_list):
    """One R_init (3 x 3 x n_b) per problem -> the concatenation of their column-major blocks; refusals name the problem."""
    if isinstance(R_init_list, (str, bytes)) or not hasattr(R_init_list, "__len__") or len(R_init_list) != len(probs):
        got = len(R_init_list) if hasattr(R_init_list, "__len__") else type(R_init_list).__name__
        raise ValueError(f"R_init_list must hold one R_init per problem ({len(probs)}), not {got}")
    parts = []
    for b, (q, R) in enumerate(zip(probs, R_init_list)):
        R = np.asarray(R, dtype=np.float64)
        if R.shape != (3, 3, q.n):
            raise ValueError(f"problem {b}: R_init must be 3 x 3 x {q.n}, not {' x '.join(str(k) for k in R.shape)}")
        bad = np.flatnonzero(~np.isfinite(R).all(axis=(0, 1)))
        if bad.size:
            raise ValueError(f"problem {b}: R_init holds a non-finite entry (node {int(bad[0])})")
        parts.append(R.reshape(-1, order="F"))
    return np.concatenate(parts) if parts else np.zeros(0)


def _refine_batch_run(probs, device, S, R_init, stop_threshold, max_iters, pset=None):
    with _batch_handle(_lib.RefineBatch, probs, device, on=pset) as batch:
        return batch.run(S, R_init, stop_threshold, max_iters)


def DESC_refine_batch(problems, S_list, R_init_list, stop_threshold=1e-3, max_iters=100, device=0, return_info=False):
    """The refinement tail of DESC (Algorithms/DESC.m:265-313) on B independent small problems in one GPU launch (desc_refine_batch_*;
    the reference has no such call): ``S_list[b]`` is problem b's S_vec in the caller's edge order, ``R_init_list[b]`` its 3 x 3 x n_b
    start (what GCW gave).  Returns a list of R_est (3 x 3 x n_b): entry b is bit for bit what the refinement stage of DESC() gives for
    these inputs, and no bit of it depends on the batch around it.  With ``return_info`` a list of (R_est, info): the record of the
    single refinement (``iters``, ``score``, ``cg_iters``, ``cg_unconverged``, ``cg_residual``, ``ms_total``) plus the call's ``timings``.
    Refused (ValueError, before the device is touched): not a sequence, an empty edge list, an S_list / R_init_list of the wrong length
    or an entry of the wrong size, a negative or non-finite S entry, a non-finite R_init entry, a problem of more than
    ``_lib.refine_batch_max_n()`` nodes (solve it with DESC)."""
    _check_sequence(problems)
    pset = _resident(problems, device)
    probs, perms = _marshal_problems(problems, rotations=pset is None)
    S = _sorted_s_list(probs, perms, S_list)
    R0 = _r_init_list(probs, R_init_list)
    if not probs:
        return []
    _check_refine_batch_sizes(probs)
    outs, timings = _refine_batch_run(probs, device, S, R0, stop_threshold, max_iters, pset)
    return [(R, dict(info, timings=timings)) for R, info in outs] if return_info else [R for R, _ in outs]


def DESC_batch(problems, params, seeds=None, return_info=False, build="host", eig="lds"):
    """DESC (Algorithms/DESC.m:14: DESC_PGD, then GCW, then the reweighted Lie-algebraic refinement) on B independent small problems:
    DESC_init_batch's two passes, then the batched refinement on their S_vec and R_init -- three GPU passes for the whole batch.
    Returns a list of (R_est, R_init, S_vec); S_vec and R_init are bit for bit DESC_init_batch's.  With ``return_info`` a list of
    (R_est, R_init, S_vec, dict(pgd=..., gcw=..., refine=...)).  The batch prints nothing: ``params.verbose`` is ignored.
    ``build`` is DESC_PGD_batch's; ``eig`` is Spectral_batch's: with ``"streamed"`` or ``"auto"`` the cap of the call is the
    refinement's, ``_lib.refine_batch_max_n()`` (748) nodes.
    Refused (ValueError, before the device is touched): what DESC_init_batch refuses, and with an ``eig`` other than the default a
    problem of more than ``_lib.refine_batch_max_n()`` nodes (solve it with DESC)."""
    _check_eig(eig)
    _check_build(build)
    _check_sequence(problems)
    pset = _resident(problems, _get(params, "device", 0))
    probs, perms = _marshal_problems(problems, rotations=pset is None)
    if eig != "lds":                                 # the default's cap lies below the refinement's: nothing to check there
        _check_gcw_batch_sizes(probs, eig)
        _check_refine_batch_sizes(probs)
    init = DESC_init_batch([_Marshalled(q, perm) for q, perm in zip(probs, perms)], params, seeds=seeds, return_info=True, build=build,
                           eig=eig, _set=pset)
    if not init:
        return []
    S = np.concatenate([S_vec if perm is None else S_vec[perm] for (_, S_vec, _), perm in zip(init, perms)])
    R0 = np.concatenate([R.reshape(-1, order="F") for R, _, _ in init])
    outs, timings = _refine_batch_run(probs, int(_get(params, "device", 0)), S, R0, 1e-3, 100, pset)
    if return_info:
        return [(R, R_init, S_vec, dict(info, refine=dict(rinfo, timings=timings))) for (R, rinfo), (R_init, S_vec, info) in zip(outs, init)]
    return [(R, R_init, S_vec) for (R, _), (R_init, S_vec, _) in zip(outs, init)]


def _cemp_batch_params(CEMP_parameters, B, seeds):
    """The fields CEMP reads, checked once for the whole batch -> (beta, max_iter, nsample, seed, device, seeds)."""
    beta = _param_vec(CEMP_parameters, "reweighting", "CEMP_parameters")
    max_iter, nsample = _get(CEMP_parameters, "max_iter"), _get(CEMP_parameters, "nsample")
    if max_iter is None or int(max_iter) < 0:
        raise ValueError("CEMP_parameters.max_iter must be an integer >= 0")
    if nsample is None or int(nsample) < 1:
        raise ValueError("CEMP_parameters.nsample must be an integer >= 1")
    seeds = _check_seeds(seeds, B)
    return beta, int(max_iter), int(nsample), int(_get(CEMP_parameters, "seed", 0)), int(_get(CEMP_parameters, "device", 0)), seeds


def _check_cemp_batch_degrees(probs):
    """The batched sampler's staging cap (neighbours of one node), checked before the device is touched."""
    cap = _lib.cemp_batch_max_degree()
    for b, q in enumerate(probs):
        deg = np.bincount(q.ind_i, minlength=q.n) + np.bincount(q.ind_j, minlength=q.n)
        v = int(np.argmax(deg))
        if deg[v] > cap:
            raise ValueError(f"problem {b}: node {v} has {int(deg[v])} neighbours, more than the {cap} the batched sampler stages per row: "
                             "solve it with CEMP")


def _check_mst_batch(probs):
    """The tree kernel's size cap and connectivity (a host union-find of the library), checked before the device is touched."""
    with _invalid_as_value_error():
        _lib.mst_batch_check(probs)


def _mst_batch_run(probs, S, device, pset=None):
    """The batched tree step on a list of ProblemArrays, or on the resident set ``pset`` they mirror."""
    return _lib.mst_batch_run_on(pset, S) if pset is not None else _lib.mst_batch_run(probs, S, device)


def _unsort(S, perm):
    if perm is None:
        return S
    out = np.empty_like(S)
    out[perm] = S
    return out


def CEMP_batch(problems, CEMP_parameters, seeds=None, return_info=False, _set=None):
    """CEMP (Algorithms/CEMP.m:24) on B independent small problems in one GPU pass (desc_cemp_batch_*; the reference has no such call).

    ``problems`` as for DESC_PGD_batch; one ``CEMP_parameters`` for the whole batch (``max_iter``, ``reweighting``, ``nsample``, optional
    ``seed`` / ``device``); ``seeds`` an optional sequence of per-problem sampling seeds.  Returns a list of SVec (caller's edge order):
    entry b is bit for bit ``CEMP(Ind_b, RijMat_b, CEMP_parameters)`` with that problem's seed, and no bit of it depends on the batch
    around it.  With ``return_info`` a list of (SVec, dict) carrying the call's ``timings``.

    Refused (ValueError, before the device is touched): not a sequence, an empty edge list, a ``seeds`` list of the wrong length,
    ``nsample < 1``, ``max_iter < 0``, a missing or empty ``reweighting``, a node of more neighbours than
    ``_lib.cemp_batch_max_degree()`` (solve that problem with CEMP)."""
    _check_sequence(problems)
    beta, max_iter, nsample, seed, device, seeds = _cemp_batch_params(CEMP_parameters, len(problems), seeds)
    pset = _set if _set is not None else _resident(problems, device)
    probs, perms = _marshal_problems(problems, rotations=pset is None)
    if not probs:
        return []
    _check_cemp_batch_degrees(probs)
    with _batch_handle(_lib.CempBatch, probs, nsample, seed, seeds, device, on=pset) as batch:
        outs, timings = batch.run(beta, max_iter)
    S = [_unsort(o, perm) for o, perm in zip(outs, perms)]
    return [(s, dict(timings=timings)) for s in S] if return_info else S


def CEMP_GCW_batch(problems, CEMP_parameters, seeds=None, return_info=False, eig="lds"):
    """CEMP_GCW (Algorithms/CEMP_GCW.m) on B independent small problems: CEMP_batch's pass, then the batched eigen-solve with the host
    weights 1/(SVec + 1e-8) and normalised rows (CEMP_GCW.m:144-146) -- two GPU passes for the whole batch.  Returns a list of R_est
    (3 x 3 x n_b); with ``return_info`` a list of (R_est, SVec, dict(cemp=..., gcw=...)), SVec bit for bit CEMP_batch's.
    ``eig`` is Spectral_batch's.
    Refused (ValueError, before the device is touched): what CEMP_batch refuses, an ``eig`` other than ``"lds"`` / ``"streamed"`` /
    ``"auto"``, and a problem of more nodes than the cap of ``eig`` (``_lib.gcw_batch_max_n()`` by default; solve it with CEMP_GCW)."""
    _check_eig(eig)
    _check_sequence(problems)
    device = _cemp_batch_params(CEMP_parameters, len(problems), seeds)[4]
    pset = _resident(problems, device)
    probs, perms = _marshal_problems(problems, rotations=pset is None)
    if not probs:
        return []
    _check_cemp_batch_degrees(probs)
    _check_gcw_batch_sizes(probs, eig)
    cemp = CEMP_batch([_Marshalled(q, perm) for q, perm in zip(probs, perms)], CEMP_parameters, seeds=seeds, return_info=True, _set=pset)
    # CEMP_batch gave SVec in the caller's order; the eigen-solve takes the library's
    w = np.concatenate([1.0 / ((S if perm is None else S[perm]) + 1e-8) for (S, _), perm in zip(cemp, perms)])      # CEMP_GCW.m:144
    outs, timings = _gcw_batch_run(probs, device, eig, pset, weights=w, normalize_rows=True)
    if return_info:
        return [(R, S, dict(cemp=ci, gcw=dict(info, timings=timings))) for (R, info), (S, ci) in zip(outs, cemp)]
    return [R for R, _ in outs]


def MST_batch(problems, S_list, device=0, return_info=False, _set=None):
    """The tree step of MPLS (Algorithms/MPLS.m:160-193, as MST()) on B independent small problems in one GPU launch
    (desc_mst_batch_run): ``S_list[b]`` is problem b's SVec in the caller's edge order.  Returns a list of R (3 x 3 x n_b): entry b is
    bit for bit ``MST(Ind_b, RijMat_b, S_b)``.  With ``return_info`` a list of (R, dict(tree_edges=..., timings=...)), ``tree_edges`` the
    0-based rows of the caller's ``Ind`` that form the tree (ascending), as MST() returns them.
    Refused (ValueError, before the device is touched): not a sequence, an empty edge list, an S_list of the wrong length or an entry of
    the wrong size or holding a non-finite value, a problem of more than ``_lib.mst_batch_max_n()`` nodes (solve it with MST), a
    disconnected problem (a node id in 1..max(Ind) that no edge touches counts as a component)."""
    _check_sequence(problems)
    pset = _set if _set is not None else _resident(problems, device)
    probs, perms = _marshal_problems(problems, rotations=pset is None)
    S = _sorted_s_list(probs, perms, S_list, "SVec", np.isfinite,
                       lambda q, perm, t: f"SVec entry {int(t if perm is None else perm[t])} is not finite")
    if not probs:
        return []
    _check_mst_batch(probs)
    with _invalid_as_value_error():
        outs, timings = _mst_batch_run(probs, S, device, pset)
    if not return_info:
        return [R for R, _ in outs]
    return [(R, dict(tree_edges=tree if perm is None else np.sort(perm[tree]), timings=timings)) for (R, tree), perm in zip(outs, perms)]


def CEMP_MST_batch(problems, CEMP_parameters, seeds=None, return_info=False):
    """The CEMP+MST initialisation (MPLS.m:36-193, the "CEMP+MST" row of Demo/compare_algorithms.m) on B independent small problems:
    CEMP_batch, then MST_batch on its SVec.  Returns a list of R_init (3 x 3 x n_b); with ``return_info`` a list of
    (R_init, SVec, dict(cemp=..., mst=...)).  Refused (ValueError, before the device is touched): what CEMP_batch and MST_batch refuse."""
    _check_sequence(problems)
    device = _cemp_batch_params(CEMP_parameters, len(problems), seeds)[4]
    pset = _resident(problems, device)
    probs, perms = _marshal_problems(problems, rotations=pset is None)
    if not probs:
        return []
    _check_cemp_batch_degrees(probs)
    _check_mst_batch(probs)
    marshalled = [_Marshalled(q, perm) for q, perm in zip(probs, perms)]
    cemp = CEMP_batch(marshalled, CEMP_parameters, seeds=seeds, return_info=True, _set=pset)
    mst = MST_batch(marshalled, [S for S, _ in cemp], device=device, return_info=True, _set=pset)
    if return_info:
        return [(R, S, dict(cemp=ci, mst=mi)) for (R, mi), (S, ci) in zip(mst, cemp)]
    return [R for R, _ in mst]


def _mpls_batch_params(MPLS_parameters):
    """The fields the MPLS loop reads, checked once for the whole batch -> (stop_threshold, max_iter, beta, tau, alpha)."""
    beta = _param_vec(MPLS_parameters, "reweighting", "MPLS_parameters")
    tau = _param_vec(MPLS_parameters, "thresholding", "MPLS_parameters")
    alpha = _param_vec(MPLS_parameters, "cycle_info_ratio", "MPLS_parameters")
    stop_threshold, max_iter = _get(MPLS_parameters, "stop_threshold"), _get(MPLS_parameters, "max_iter")
    if stop_threshold is None:
        raise ValueError("MPLS_parameters.stop_threshold is required")
    if max_iter is None:
        raise ValueError("MPLS_parameters.max_iter is required")
    return float(stop_threshold), int(max_iter), beta, tau, alpha


def MPLS_batch(problems, CEMP_parameters, MPLS_parameters, seeds=None, return_info=False):
    """MPLS (Algorithms/MPLS.m:31, the "MPLS" row of Demo/compare_algorithms.m) on B independent small problems: ONE batched CEMP handle
    runs the rounds, the batched tree kernel turns their SVec into R_init, and the MPLS loop of every problem runs in one launch on the
    same handle, whose sampled cycles stay resident (desc_cemp_batch_*, desc_mst_batch_run, desc_mpls_batch_run; the reference has no
    such call).

    ``problems`` as for DESC_PGD_batch; one ``CEMP_parameters`` and one ``MPLS_parameters`` for the whole batch, with the fields MPLS()
    reads; ``seeds`` an optional sequence of per-problem sampling seeds.  Returns a list of (R_est, R_init): entry b is bit for bit
    ``MPLS(Ind_b, RijMat_b, dict(CEMP_parameters, seed=seed_b), MPLS_parameters)``, and no bit of it depends on the batch around it.
    With ``return_info`` a list of (R_est, R_init, dict(SVec=..., cemp=..., mst=..., mpls=...)): CEMP's SVec in the caller's edge
    order, the timings of the first two passes, and the loop's record (``iters``, ``score``, ``cg_iters``, ``cg_unconverged``,
    ``cg_residual``, ``m_pos``, ``timings``).  The batch prints nothing: ``verbose`` is ignored.

    Refused (ValueError, before the device is touched, naming the problem): what CEMP_MST_batch refuses; a missing or empty
    ``MPLS_parameters.reweighting``, ``.thresholding`` or ``.cycle_info_ratio``; a missing ``stop_threshold`` or ``max_iter``; a problem
    of more than ``_lib.mpls_batch_max_n()`` nodes (solve it with MPLS)."""
    _check_sequence(problems)
    cemp_beta, cemp_max_iter, nsample, seed, device, seeds = _cemp_batch_params(CEMP_parameters, len(problems), seeds)
    stop_threshold, max_iter, beta, tau, alpha = _mpls_batch_params(MPLS_parameters)
    pset = _resident(problems, device)
    probs, perms = _marshal_problems(problems, rotations=pset is None)
    if not probs:
        return []
    _check_cemp_batch_degrees(probs)
    _check_mst_batch(probs)
    _check_batch_sizes(probs, _lib.mpls_batch_max_n(), "per-node state of the MPLS loop", "MPLS")
    with _batch_handle(_lib.CempBatch, probs, nsample, seed, seeds, device, on=pset) as batch:
        S_list, cemp_tm = batch.run(cemp_beta, cemp_max_iter)
        S = np.concatenate(S_list)                                   # the library's edge order, as both later passes take it
        with _invalid_as_value_error():
            mst, mst_tm = _mst_batch_run(probs, S, device, pset)
            R0 = np.concatenate([R.reshape(-1, order="F") for R, _ in mst])
            outs, mpls_tm = batch.mpls_run(S, R0, stop_threshold, max_iter, beta, tau, alpha)
    if not return_info:
        return [(R, R_init) for (R, _), (R_init, _) in zip(outs, mst)]
    return [(R, R_init, dict(SVec=_unsort(S_b.copy(), perm), cemp=dict(timings=cemp_tm),
                             mst=dict(tree_edges=tree if perm is None else np.sort(perm[tree]), timings=mst_tm),
                             mpls=dict(info, timings=mpls_tm)))
            for (R, info), (R_init, tree), S_b, perm in zip(outs, mst, S_list, perms)]


def _irls_batch(mode, name, problems, SIGMA, MaxIterations, device, return_info):
    _check_sequence(problems)
    mi = np.atleast_1d(np.asarray(MaxIterations, dtype=np.float64)).reshape(-1)
    if mi.size != 2:
        raise ValueError("MaxIterations must have two entries [L1, IRLS]")
    sigma = 5.0 if SIGMA is None or np.size(SIGMA) == 0 else float(SIGMA)
    pset = _resident(problems, device)
    # a set holds 3 x 3 x m blocks by construction: its items' RijMat (a fetch, for a generated set) is not touched
    for b, item in enumerate(problems if pset is None else ()):
        if isinstance(item, _Marshalled):
            continue
        try:
            R = np.asarray(item.RijMat if hasattr(item, "RijMat") else item[1])
        except (TypeError, IndexError, KeyError):
            continue                                                 # _marshal_problems has the words for it
        if R.ndim == 2 and R.shape[0] == 4:
            raise ValueError(f"problem {b}: the quaternion form of RR (4 x m) is not supported: pass RijMat as 3 x 3 x m rotation matrices")
    probs, perms = _marshal_problems(problems, rotations=pset is None)
    if not probs:
        return []
    single = "IRLS_GM / IRLS_L12"
    _check_batch_sizes(probs, _lib.irls_batch_max_n(), "per-node state of the L1 stage", single)
    for b, (q, perm) in enumerate(zip(probs, perms)):                # connectivity: the host half of the spanning-tree start
        with _invalid_as_value_error():
            reached = _lib.irls_tree_sequence(q, perm)[2]
        if reached < q.n:
            raise ValueError(f"problem {b}: the graph is not connected ({reached} of {q.n} nodes reached from node 1): solve it with {single}")
    with _batch_handle(_lib.IrlsBatch, probs, perms, int(device), on=pset) as batch:
        outs, timings = batch.run(mode, sigma, int(mi[0]), int(mi[1]))
    warned = [b for b, (_, _, info) in enumerate(outs) if info["warned_edges"]]
    if warned:
        import warnings
        warnings.warn(f"{name}: edge rotations with all three singular values off 1 by >= 0.01 were projected to SO(3) in problems "
                      + ", ".join(f"{b} ({outs[b][2]['warned_edges']})" for b in warned), RuntimeWarning, stacklevel=3)
    if not return_info:
        return [R for R, _, _ in outs]
    result = []
    for R, R_l1, info in outs:
        info = {k: v for k, v in info.items() if not k.startswith("ms_")}
        info["R_l1"] = R_l1
        info["timings"] = timings
        result.append((R, info))
    return result


def IRLS_GM_batch(problems, SIGMA=5, MaxIterations=(10, 100), device=0, return_info=False):
    """IRLS_GM (Algorithms/IRLS_GM.m, the "IRLS-GM" row of Demo/compare_algorithms.m) on B independent small, connected problems in two
    GPU launches (desc_irls_batch_*; the reference has no such call): one projects the edges of all problems, one runs a workgroup per
    problem from the spanning-tree start through the L1 loop and the reweighted loop.

    ``problems`` as for DESC_PGD_batch; one ``SIGMA`` (degrees) and one ``MaxIterations`` = (L1, IRLS) for the whole batch.  Returns a
    list of R (3 x 3 x n_b).  With ``return_info`` a list of (R, info): ``info`` has the keys of ``IRLS_GM(..., return_info=True)``
    -- ``R_l1``, the iteration counts and scores, the primal-dual and PCG counts, ``warned_edges``, ``comp_nodes`` / ``comp_edges`` --
    except the per-stage milliseconds, which are the batch's, under ``timings``.  Entry b is bit for bit
    ``IRLS_GM(RijMat_b, Ind_b, SIGMA=..., MaxIterations=..., return_info=True)`` in all of them, and no bit of it depends on the
    batch around it.  The call prints nothing; projected ("warned") edges are reported in one RuntimeWarning naming the problems.

    Refused (ValueError, before the device is touched, naming the problem): not a sequence, an empty edge list, ``MaxIterations``
    without two entries, the 4 x m quaternion form of RijMat, a problem that is not connected or has more than
    ``_lib.irls_batch_max_n()`` nodes (solve it with IRLS_GM / IRLS_L12; component extraction stays with the single call).  There is no
    ``Rinit``.  An edge rotation with det <= 0, or with all three singular values off 1 by >= 0.1, raises DescError naming the problem
    and the 1-based row of its ``Ind`` (the lowest problem, the smallest row in it)."""
    return _irls_batch(_lib.IRLS_GM, "IRLS_GM_batch", problems, SIGMA, MaxIterations, device, return_info)


def IRLS_L12_batch(problems, SIGMA=5, MaxIterations=(10, 100), device=0, return_info=False):
    """IRLS_L12 (Algorithms/IRLS_L12.m, the "IRLS-L0.5" row) on B independent small, connected problems: as IRLS_GM_batch with
    Utils/L12.m's weights in the reweighted stage (SIGMA is accepted and unused, as in the reference); entry b is bit for bit
    ``IRLS_L12(RijMat_b, Ind_b, ...)``."""
    return _irls_batch(_lib.IRLS_L12, "IRLS_L12_batch", problems, SIGMA, MaxIterations, device, return_info)


def linprog_sij_batch(problems, params=None, seeds=None, rotations=True, return_info=False, eig="lds"):
    """linprog_sij (Algorithms/linprog_sij.m:16) on B independent small problems: the LP of every problem in one batched PDHG loop
    (desc_lp_batch_*: two launches per step and one 4-byte read-back per check for the whole batch), then the row-normalised weighted
    spectral step with weights exp(-5 S_vec) on the batched eigen-solve and the refinement with maxIters = 200 on the batched
    refinement -- three batched handles (the reference has no such call).

    ``problems`` as for DESC_PGD_batch; one ``params`` for the whole batch with the fields of linprog_sij: ``seed``, ``device``, ``tol``,
    ``max_iter``, ``check_every``, ``restart``, ``return_dual`` and ``nsample`` -- None (the rule of :43, evaluated per problem), one int,
    or a sequence of B ints; ``seeds`` an optional sequence of per-problem sampling seeds (default: ``params.seed`` for every problem).
    Returns a list of (R_est, S_vec), S_vec in the caller's edge order: entry b's S_vec is bit for bit
    ``linprog_sij(Ind_b, RijMat_b, dict(params, seed=seed_b, nsample=nsample_b))``'s, each problem stops at its own step, and no bit of
    it depends on the batch around it.  With ``return_info`` a list of (R_est, S_vec, info) with linprog_sij's keys ``lp``,
    ``pos_edges``, ``k``, ``R_gcw``, ``spectral``, ``refine`` and, with ``return_dual``, ``y``.  ``rotations=False`` runs the LP only and
    returns a list of S_vec, or of (S_vec, info).  The batch prints nothing: ``verbose`` is ignored.

    Refused (ValueError, before the device is touched, naming the problem): not a sequence, an empty edge list, ``nsample < 0``, a
    ``seeds`` or ``nsample`` sequence of the wrong length, a node of more neighbours than ``_lib.cemp_batch_max_degree()`` (the batched
    sampler's cap; solve it with linprog_sij), a batch whose LP rows reach 2^31 (split the batch), an ``eig`` other than ``"lds"`` /
    ``"streamed"`` / ``"auto"``, and with ``rotations=True`` a problem of more than ``_lib.gcw_batch_max_n()`` nodes (solve it with
    linprog_sij, or pass rotations=False for S_vec alone).  ``eig`` is Spectral_batch's: with ``"streamed"`` or ``"auto"`` the cap of
    the rotations is the refinement's, ``_lib.refine_batch_max_n()`` (748) nodes."""
    _check_eig(eig)
    _check_sequence(problems)
    params = {} if params is None else params
    B = len(problems)
    seeds = _check_seeds(seeds, B)
    nsample = _get(params, "nsample")
    if nsample is not None and np.ndim(nsample) != 0 and len(nsample) != B:
        raise ValueError(f"nsample must hold one entry per problem ({B}), not {len(nsample)}")
    p = _lib.default_lp_params()
    for name, cast in (("tol", float), ("max_iter", int), ("check_every", int), ("restart", int)):
        if _get(params, name) is not None:
            setattr(p, name, cast(_get(params, name)))
    p.verbose = 0
    want_y, device = bool(_get(params, "return_dual", False)), int(_get(params, "device", 0))
    if seeds is None:
        seeds = [int(_get(params, "seed", 0))] * B
    pset = _resident(problems, device)
    if B == 0:
        return []
    probs, perms = _marshal_problems(problems)
    try:
        _lib.lp_batch_plan(probs, nsample)                               # create's refusals, on the host
    except _lib.DescError as e:
        if e.code in (_lib.ERR_INVALID, _lib.ERR_TOO_LARGE):
            raise ValueError(str(e).split(": ", 1)[-1]) from None
        raise
    if rotations:
        instead = "linprog_sij, or pass rotations=False for S_vec alone"
        _check_gcw_batch_sizes(probs, eig, instead)
        if eig != "lds":                             # the default's cap lies below the refinement's: nothing to check there
            _check_batch_sizes(probs, _lib.refine_batch_max_n(), "per-node state of the refinement", instead)
    with _batch_handle(_lib.LpBatch, probs, nsample, seeds, device) as batch:
        outs, lp_tm = batch.run(p, want_y=want_y)
        samples = batch.samples() if return_info else None
    S_list = [_unsort(S, perm) for (S, _, _), perm in zip(outs, perms)]
    infos = None
    if return_info:
        infos = []
        for (S, y, lp), smp, perm in zip(outs, samples, perms):
            info = dict(lp=dict(lp, timings=lp_tm), pos_edges=smp["pos_edges"] if perm is None else perm[smp["pos_edges"]], k=smp["k"])
            if want_y:
                info["y"] = y
            infos.append(info)
    if not rotations:
        return [(S, info) for S, info in zip(S_list, infos)] if return_info else S_list
    S = np.concatenate([S for S, _, _ in outs])                          # the library's edge order, as both later passes take it
    gcw, gcw_tm = _gcw_batch_run(probs, device, eig, pset, weights=np.exp(-5.0 * S), normalize_rows=True)   # :154-174, beta_T = 5
    R0 = np.concatenate([R.reshape(-1, order="F") for R, _ in gcw])
    ref, ref_tm = _refine_batch_run(probs, device, S, R0, 1e-3, 200, pset)                                        # :176-351
    if not return_info:
        return [(R, S_b) for (R, _), S_b in zip(ref, S_list)]
    for info, (R_gcw, sinfo), (_, rinfo) in zip(infos, gcw, ref):
        info.update(R_gcw=R_gcw, spectral=dict(sinfo, timings=gcw_tm), refine=dict(rinfo, timings=ref_tm))
    return [(R, S_b, info) for (R, _), S_b, info in zip(ref, S_list, infos)]


def _run_with_plots(solver, p, params, prob, dprob, perm, verbose, adam=None):
    """params.make_plots = true (DESC_PGD.m:235-239): after every iteration the error of S_vec against params.ErrVec and
    the rotation error of GCW(S_vec) against params.R_orig (GlobalSOdCorrectRight = the alignment of Rotation_Alignment).
    A composition of device rows: one sweep, one S_vec download and one GCW eigen-solve per iteration."""
    own = None
    if not isinstance(dprob, _lib.DeviceProblem):
        own = dprob = _lib.DeviceProblem(prob, p.device)
    ErrVec = np.asarray(_get(params, "ErrVec"), dtype=np.float64).reshape(-1)
    R_orig = np.asarray(_get(params, "R_orig"), dtype=np.float64)
    if perm is not None:
        ErrVec = ErrVec[perm]
    try:
        out = solver.run_traced(p, dprob, ErrVec, adam=adam)                     # desc_pgd_run_traced: :236-237 for every iteration
    finally:
        if own is not None:
            own.free()
    mse_means, mse_medians = [], []
    for R_est in out.pop("R_est_all"):
        _, _, mean_e, med_e = Rotation_Alignment(R_est, R_orig)                                  # :238
        mse_means.append(mean_e); mse_medians.append(med_e)
    svec_errors = out["svec_errors"]
    k = out["iters_run"]
    out["svec_errors"] = np.array(svec_errors[:k]); out["MSE_means"] = np.array(mse_means[:k]); out["MSE_medians"] = np.array(mse_medians[:k])
    return out


def _run_external(solver, p, G, params, prob, dprob, perm, verbose, make_plots):
    """The loop of DESC_PGD.m:182-257 around a plugin the library does not know (Solver.run_external): G.GetStep is called once per
    iteration, exactly iters_run times, with grad_long in the cycle order of the SORTED problem (an unsorted Ind permutes the edge vectors
    only: segment l belongs to the l-th edge with cycles in (i, j) order).  A plugin with ``device_tensors = True`` is given and returns
    float64 torch tensors on the solver's GPU; any other plugin NumPy arrays.  What GetStep raises propagates unchanged.  With
    make_plots, :235-239 run after every applied step and give the keys of _run_with_plots."""
    line = None
    if verbose:
        def line(it, avg, obj):
            print("iter %d: average change in S_vec %f, objective value: %f" % (it, avg, obj), flush=True)      # DESC_PGD.m:241
    after = own = None
    if make_plots:
        if not isinstance(dprob, _lib.DeviceProblem):
            own = dprob = _lib.DeviceProblem(prob, p.device)
        ErrVec = np.asarray(_get(params, "ErrVec"), dtype=np.float64).reshape(-1)
        R_orig = np.asarray(_get(params, "R_orig"), dtype=np.float64)
        if perm is not None:
            ErrVec = ErrVec[perm]
        svec_errors, mse_means, mse_medians = [], [], []

        def after(it):
            S = solver.download()["S_vec"]
            svec_errors.append(float(np.mean(np.abs(ErrVec - S))))                               # :236
            R_est, _ = _lib.gcw_run(dprob, S)                                                    # :237
            _, _, mean_e, med_e = Rotation_Alignment(R_est, R_orig)                              # :238
            mse_means.append(mean_e); mse_medians.append(med_e)
    try:
        out = solver.run_external(p, G.GetStep, device_tensors=bool(getattr(G, "device_tensors", False)), device=p.device,
                                  progress=line, after_step=after)
    finally:
        if own is not None:
            own.free()
    if make_plots:
        k = out["iters_run"]
        out["svec_errors"] = np.array(svec_errors[:k]); out["MSE_means"] = np.array(mse_means[:k]); out["MSE_medians"] = np.array(mse_medians[:k])
    return out


def plot_convergence(info, path=None):
    """The 2 x 2 figure of DESC.m:315-344 from the traces of a make_plots run (matplotlib, if it is installed)."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return None
    fig, ax = plt.subplots(2, 2, figsize=(10, 8))
    for a, key, title, yl in ((ax[0, 0], "svec_errors", "Convergence of Corruption Estimate Vector (S_vec, sampled)", "Average distance to true corruption"),
                              (ax[0, 1], "obj", "Convergence of Objective Function (sampled)", "Value of Objective Function"),
                              (ax[1, 0], "MSE_means", "Convergence of Rotation Estimate, Mean (sampled)", "Mean Error in R estimate (degrees)"),
                              (ax[1, 1], "MSE_medians", "Convergence of Rotation Estimate, Median (sampled)", "Median Error in R estimate (degrees)")):
        a.plot(np.arange(1, len(info[key]) + 1), info[key]); a.set_title(title, fontsize=9); a.set_xlabel("Iteration number"); a.set_ylabel(yl)
    fig.tight_layout()
    if path:
        fig.savefig(path)
    return fig


def Spectral(Ind, RijMat, device=0, return_info=False):
    """R_est = Spectral(Ind, RijMat) -- Algorithms/Spectral.m:15.  3 x 3 x n rotations, defined
    up to one global right rotation (use Rotation_Alignment to compare)."""
    n, ii, jj, rij, perm = marshal_edges(Ind, RijMat)
    prob = _lib.ProblemArrays(n, ii, jj, rij)
    R, info = _lib.spectral_run(prob, None, False, device=device)
    return (R, info) if return_info else R


def GCW(Ind, AdjMat, RijMat, S_vec, device=0, return_info=False):
    """R_est = GCW(Ind, AdjMat, RijMat, S_vec) -- Utils/GCW.m:1.  ``AdjMat`` is accepted for
    signature compatibility and not used (it is implied by ``Ind``)."""
    n, ii, jj, rij, perm = marshal_edges(Ind, RijMat)
    S = np.asarray(S_vec, dtype=np.float64).reshape(-1)
    if S.shape[0] != ii.shape[0]:
        raise ValueError("S_vec must have one entry per edge")
    if perm is not None:
        S = S[perm]
    w = 1.0 / (S * np.sqrt(S) + 1e-8)                         # GCW.m:20: SVec.^(1.5) (sqrt form: 5x cheaper than pow; S >= 0)
    prob = _lib.ProblemArrays(n, ii, jj, rij)
    R, info = _lib.spectral_run(prob, w, True, device=device)
    return (R, info) if return_info else R


def CEMP(Ind, RijMat, CEMP_parameters, return_info=False):
    """SVec = CEMP(Ind, RijMat, CEMP_parameters) -- Algorithms/CEMP.m:24.  Fields read:
    ``max_iter``, ``reweighting``, ``nsample`` (``gcw_beta`` is ignored, as in the reference);
    optional ``seed`` / ``device`` (not in the reference)."""
    n, ii, jj, rij, perm = marshal_edges(Ind, RijMat)
    prob = _lib.ProblemArrays(n, ii, jj, rij)
    beta = np.atleast_1d(np.asarray(_get(CEMP_parameters, "reweighting"), dtype=np.float64))
    if _get(CEMP_parameters, "verbose", False):
        for line in ("sampling 3-cycles", "Sampling Finished!", "Initializing", "Initialization completed!",
                     "Reweighting Procedure Started ..."):           # CEMP.m:45,67,68,104,105
            print(line)
    S, ms = _lib.cemp_run(prob, beta, int(_get(CEMP_parameters, "max_iter")), int(_get(CEMP_parameters, "nsample")),
                          int(_get(CEMP_parameters, "seed", 0)), int(_get(CEMP_parameters, "device", 0)))
    if perm is not None:
        out = np.empty_like(S); out[perm] = S; S = out
    return (S, dict(ms_total=ms)) if return_info else S


def _param_vec(params, name, what):
    v = _get(params, name)
    if v is None:
        raise ValueError(f"{what}.{name} is required")
    v = np.atleast_1d(np.asarray(v, dtype=np.float64)).reshape(-1)
    if v.size == 0:
        raise ValueError(f"{what}.{name} needs at least one entry")
    return v


def MPLS(Ind, RijMat, CEMP_parameters, MPLS_parameters, return_info=False):
    """[R_est, R_init] = MPLS(Ind, RijMat, CEMP_parameters, MPLS_parameters) -- Algorithms/MPLS.m:31.

    ``R_init`` is the CEMP+MST initialisation (MPLS.m:160-193), ``R_est`` the result of the cycle-reweighted Lie-algebraic
    averaging (:196-254).  Fields read, as Demo/compare_algorithms.m:26-36 sets them: ``CEMP_parameters.max_iter``,
    ``.reweighting``, ``.nsample``; ``MPLS_parameters.stop_threshold``, ``.max_iter``, ``.reweighting``, ``.thresholding``,
    ``.cycle_info_ratio``.  Optional (not in the reference): ``seed`` (cycle sampling), ``device`` and ``verbose`` (the reference's
    disp / fprintf lines; default off), read from CEMP_parameters.  One device problem serves all three stages.  With
    ``return_info`` also a dict: iterations, score, PCG counts, m_pos, per-stage milliseconds and CEMP's ``SVec`` (caller's order)."""
    n, ii, jj, rij, perm = marshal_edges(Ind, RijMat)
    if ii.shape[0] == 0:
        raise ValueError("empty edge list")
    cemp_beta = _param_vec(CEMP_parameters, "reweighting", "CEMP_parameters")
    beta = _param_vec(MPLS_parameters, "reweighting", "MPLS_parameters")
    tau = _param_vec(MPLS_parameters, "thresholding", "MPLS_parameters")
    alpha = _param_vec(MPLS_parameters, "cycle_info_ratio", "MPLS_parameters")
    verbose = bool(_get(CEMP_parameters, "verbose", False))
    prob = _lib.ProblemArrays(n, ii, jj, rij)
    dprob = _lib.DeviceProblem(prob, int(_get(CEMP_parameters, "device", 0)))
    try:
        if verbose:
            import sys
            sys.stdout.flush()
        R_est, R_init, S, info = _lib.mpls_run(dprob, cemp_beta, int(_get(CEMP_parameters, "max_iter")), int(_get(CEMP_parameters, "nsample")),
                                               float(_get(MPLS_parameters, "stop_threshold")), int(_get(MPLS_parameters, "max_iter")),
                                               beta, tau, alpha, seed=int(_get(CEMP_parameters, "seed", 0)), verbose=verbose)
    finally:
        dprob.free()
    if return_info:
        if perm is not None:
            out = np.empty_like(S); out[perm] = S; S = out
        info["SVec"] = S
        return R_est, R_init, info
    return R_est, R_init


def MST(Ind, RijMat, SVec, device=0, return_info=False):
    """R_est = the tree step of MPLS (Algorithms/MPLS.m:160-193): the minimum spanning tree of the graph weighted by SVec + 1,
    rotations multiplied along it from node 1 (R_1 = I).

    This follows MPLS.m:162 (weights ``SVec + 1``), not ``Utils/MST.m``, whose ``sparse`` call drops the edges with
    ``SVec == 0``.  Ties of the computed ``SVec + 1`` are broken by the edge's (i, j) order, so the tree is unique.  A graph that
    is not connected raises DescError.  With ``return_info`` also a dict whose ``tree_edges`` are the 0-based rows of the caller's
    ``Ind`` that form the tree (ascending)."""
    n, ii, jj, rij, perm = marshal_edges(Ind, RijMat)
    if ii.shape[0] == 0:
        raise ValueError("empty edge list")
    S = np.asarray(SVec, dtype=np.float64).reshape(-1)
    if S.shape[0] != ii.shape[0]:
        raise ValueError("SVec must have one entry per edge")
    if perm is not None:
        S = S[perm]
    prob = _lib.ProblemArrays(n, ii, jj, rij)
    R, tree = _lib.mst_run(prob, S, device=device)
    if not return_info:
        return R
    rows = np.sort(perm[tree]) if perm is not None else tree
    return R, dict(tree_edges=rows)


def CEMP_GCW(Ind, RijMat, CEMP_parameters, return_info=False):
    """R_est = CEMP_GCW(Ind, RijMat, CEMP_parameters) -- Algorithms/CEMP_GCW.m: CEMP's SVec, then the row-normalised weighted
    spectral step with the weights 1/(SVec + 1e-8) of CEMP_GCW.m:144 (GCW() uses 1/(SVec^1.5 + 1e-8), GCW.m:20).  Both stages
    run on one device problem."""
    n, ii, jj, rij, perm = marshal_edges(Ind, RijMat)
    if ii.shape[0] == 0:
        raise ValueError("empty edge list")
    beta = _param_vec(CEMP_parameters, "reweighting", "CEMP_parameters")
    prob = _lib.ProblemArrays(n, ii, jj, rij)
    dprob = _lib.DeviceProblem(prob, int(_get(CEMP_parameters, "device", 0)))
    try:
        S, ms = _lib.cemp_run(dprob, beta, int(_get(CEMP_parameters, "max_iter")), int(_get(CEMP_parameters, "nsample")),
                              int(_get(CEMP_parameters, "seed", 0)))
        R, info = _lib.spectral_run(dprob, 1.0 / (S + 1e-8), True)                               # CEMP_GCW.m:144-146
    finally:
        dprob.free()
    return (R, dict(info, ms_cemp=ms)) if return_info else R


def _irls(mode, RijMat, Ind, Rinit, SIGMA, MaxIterations, device, verbose, return_info):
    R = np.asarray(RijMat)
    if R.ndim == 2 and R.shape[0] == 4:
        raise ValueError("the quaternion form of RR (4 x m) is not supported: pass RijMat as 3 x 3 x m rotation matrices")
    mi = np.atleast_1d(np.asarray(MaxIterations, dtype=np.float64)).reshape(-1)
    if mi.size != 2:
        raise ValueError("MaxIterations must have two entries [L1, IRLS]")
    sigma = 5.0 if SIGMA is None or np.size(SIGMA) == 0 else float(SIGMA)
    n, ii, jj, rij, perm = marshal_edges(Ind, R)
    if ii.shape[0] == 0:
        raise ValueError("empty edge list")
    if Rinit is not None and (np.ndim(Rinit) != 3 or np.shape(Rinit)[:2] != (3, 3) or np.shape(Rinit)[2] != n):
        raise ValueError("Rinit must be 3 x 3 x max(Ind(:))")
    prob = _lib.ProblemArrays(n, ii, jj, rij)
    if verbose:
        import sys
        sys.stdout.flush()
    Rout, R_l1, info = _lib.irls_run(prob, mode, int(mi[0]), int(mi[1]), sigma, R_init=Rinit, order=perm, device=device, verbose=verbose)
    if return_info:
        info["R_l1"] = R_l1
        return Rout, info
    return Rout


def IRLS_GM(RijMat, Ind, Rinit=None, SIGMA=5, MaxIterations=(10, 100), device=0, verbose=False, return_info=False):
    """R = IRLS_GM(RijMat, Ind, 'Rinit', Rinit, 'SIGMA', SIGMA, 'MaxIterations', [L1, IRLS]) -- Algorithms/IRLS_GM.m.  Note the
    reference's argument order: RijMat first.  The largest connected component of the graph is solved (others get NaN): L1
    initialisation by BoxMedianSO3Graph (spanning-tree start over the rows of Ind in the caller's order, three l1decode_pd solves
    per iteration), then RobustMeanSO3Graph's Geman-McClure reweighted averaging with SIGMA in degrees.  An edge rotation with
    det <= 0, or with all three singular values off 1 by >= 0.1, raises DescError naming the 1-based row.  ``verbose`` prints the
    reference's progress lines.  With ``return_info`` also a dict: component size, iteration counts and scores, primal-dual step and
    early-return counts, PCG totals, per-stage milliseconds and ``R_l1``, the L1 stage's estimate."""
    return _irls(_lib.IRLS_GM, RijMat, Ind, Rinit, SIGMA, MaxIterations, device, verbose, return_info)


def IRLS_L12(RijMat, Ind, Rinit=None, SIGMA=5, MaxIterations=(10, 100), device=0, verbose=False, return_info=False):
    """R = IRLS_L12(RijMat, Ind, ...) -- Algorithms/IRLS_L12.m: as IRLS_GM, with Utils/L12.m's weights min(|E|^-0.75, 1e4) in the
    reweighted stage (SIGMA is accepted and unused, as in the reference)."""
    return _irls(_lib.IRLS_L12, RijMat, Ind, Rinit, SIGMA, MaxIterations, device, verbose, return_info)


def _pgd_with_upload(Ind, RijMat, params, body):
    """DESC_PGD with the upload of the device problem overlapped (a helper thread), then body(dprob, perm, S_vec, S_sorted, info) on it."""
    n, ii, jj, rij, perm = marshal_edges(Ind, RijMat)
    if ii.shape[0] == 0:
        raise ValueError("empty edge list")
    prob = _lib.ProblemArrays(n, ii, jj, rij)
    device = int(_get(params, "device", 0))
    # Ind / RijMat / CSR index go to HBM once for all stages -- on a helper thread, while DESC_PGD builds the cycle structure (which needs
    # only the edge list): DESC_PGD asks for the device problem when it creates the solver
    import threading
    box = {}

    def _upload():
        try:
            box["dp"] = _lib.DeviceProblem(prob, device)
        except BaseException as e:      # noqa: BLE001  (re-raised on the calling thread)
            box["err"] = e

    th = threading.Thread(target=_upload)
    th.start()
    if os.environ.get("DESC_DEBUG_SERIAL_UPLOAD") == "1":       # A/B: the upload first, then the structure (as before round 4)
        th.join()

    def _dprob():
        th.join()
        if "err" in box:
            raise box["err"]
        return box["dp"]

    try:
        S_vec, info = DESC_PGD(Ind, RijMat, params, return_info=True, _marshalled=(perm, prob, _dprob))
        dprob = _dprob()
        S_sorted = S_vec if perm is None else S_vec[perm]
        return body(dprob, S_vec, S_sorted, info)
    finally:
        th.join()
        if "dp" in box:
            box["dp"].free()


def DESC(Ind, RijMat, params, return_info=False):
    """[R_est, R_init, S_vec] = DESC(Ind, RijMat, params) -- Algorithms/DESC.m:14 (the call of
    Demo/compare_algorithms.m:72): DESC_PGD (:16-261) -> GCW initialisation (:263) -> reweighted
    Lie-algebraic refinement (:265-313).  All three stages run on the GPU."""
    def body(dprob, S_vec, S_sorted, info):
        R_init, ginfo = _lib.gcw_run(dprob, S_sorted)                    # GCW.m:9-36, weights (GCW.m:20) formed on the device
        verbose = bool(_get(params, "verbose", True))
        if verbose:
            print("Rotation Initialized!"); print("Start DESC refinement ...")                # DESC.m:283-284
        R_est, rinfo = _lib.refine_run(dprob, S_sorted, R_init, verbose=verbose)
        if verbose:
            print("DONE!")                                                                    # DESC.m:313
        if return_info:
            return R_est, R_init, S_vec, dict(pgd=info, gcw=ginfo, refine=rinfo)
        return R_est, R_init, S_vec

    return _pgd_with_upload(Ind, RijMat, params, body)


def DESC_init(Ind, RijMat, params, return_info=False):
    """[R_est, S_vec] = DESC_init(Ind, RijMat, params) -- Algorithms/DESC_init.m: DESC_PGD followed by GCW, without the refinement: what
    DESC() returns as R_init and S_vec.  Both stages run on one device problem, uploaded while the cycle structure is built.  With
    ``params.make_plots`` the info dict holds DESC_PGD's traces; the two CSV files the reference appends to when plotting
    (DESC_init.m:262-263) are written only when ``params.csv_dir`` names a directory: one row of MSE_means to
    ``linear_convergence_rotation_error.csv`` and one of svec_errors to ``linear_convergence_svec_error.csv``."""
    def body(dprob, S_vec, S_sorted, info):
        R_est, ginfo = _lib.gcw_run(dprob, S_sorted)                     # DESC_init.m: R_est = GCW(Ind, AdjMat, RijMat, S_vec)
        csv_dir = _get(params, "csv_dir")
        if csv_dir is not None and bool(_get(params, "make_plots", False)):
            for name, key in (("linear_convergence_rotation_error", "MSE_means"), ("linear_convergence_svec_error", "svec_errors")):
                with open(os.path.join(str(csv_dir), name + ".csv"), "a") as f:                  # :262-263 (dlmwrite ... '-append': 5 digits)
                    f.write(",".join("%.5g" % v for v in info[key]) + "\n")
        if return_info:
            return R_est, S_vec, dict(pgd=info, gcw=ginfo)
        return R_est, S_vec

    return _pgd_with_upload(Ind, RijMat, params, body)


def linprog_sij(Ind, RijMat, params=None, return_info=False):
    """[Rest, S_vec] = linprog_sij(Ind, RijMat) -- Algorithms/linprog_sij.m:16.  Three stages on one device problem:
    the LP  min sum s_ij  s.t.  |s_ij - d_ijk| <= s_ik + s_jk on sampled 3-cycles, 0 <= s <= 1 (:16-139; a matrix-free PDHG solver on
    the GPU, desc_lp_sij_run_dev), the row-normalised weighted spectral step with weights exp(-5 S_vec) (:154-174), and the reweighted
    Lie-algebraic refinement of DESC.m:265-313 with maxIters = 200 (:176-351).  Edges without a 3-cycle keep S_vec = 1.

    Optional ``params`` fields, none of them in the reference: ``seed`` (cycle sampling; MATLAB uses its global RNG), ``device``,
    ``tol`` (1e-4), ``max_iter`` (200000), ``nsample`` (the rule of :43), ``verbose``, ``return_dual``.  With ``return_info`` a third
    result: the LP record (``lp``: nsample, m_pos, rows, iters, restarts, converged, viol, pobj, dobj, stage milliseconds),
    ``pos_edges`` (0-based rows of the caller's ``Ind`` that are LP variables, in variable order), ``k`` (m_pos x nsample sampled third
    nodes, 1-based), ``y`` (m_pos x nsample x 2 row duals, with ``return_dual``), ``R_gcw`` and the ``spectral`` / ``refine`` records.
    The LP optimum is not unique: compare solutions through viol / pobj / dobj, not element by element."""
    params = {} if params is None else params
    n, ii, jj, rij, perm = marshal_edges(Ind, RijMat)
    if ii.shape[0] == 0:
        raise ValueError("empty edge list")
    prob = _lib.ProblemArrays(n, ii, jj, rij)
    p = _lib.default_lp_params()
    p.seed = int(_get(params, "seed", 0))
    if _get(params, "tol") is not None:
        p.tol = float(_get(params, "tol"))
    if _get(params, "max_iter") is not None:
        p.max_iter = int(_get(params, "max_iter"))
    if _get(params, "nsample") is not None:
        p.nsample = int(_get(params, "nsample"))
    for name in ("check_every", "restart"):                  # test / measurement hooks
        if _get(params, name) is not None:
            setattr(p, name, int(_get(params, name)))
    verbose = _get(params, "verbose", False)
    p.verbose = int(verbose) if not isinstance(verbose, bool) else (1 if verbose else 0)
    want_y = bool(_get(params, "return_dual", False))
    if p.verbose:
        import sys
        sys.stdout.flush()
    dprob = _lib.DeviceProblem(prob, int(_get(params, "device", 0)))
    try:
        S, y, k, lpinfo = _lib.lp_sij_run(dprob, p, want_y=want_y, want_k=bool(return_info))
        if p.verbose:
            for _ in range(1000, int(lpinfo["m_pos"]) + 1, 1000):
                print("next 1000 done")                                                       # linprog_sij.m:115-117
        R_gcw, sinfo = _lib.spectral_run(dprob, np.exp(-5.0 * S), True)                       # :154-174, beta_T = 5
        Rest, rinfo = _lib.refine_run(dprob, S, R_gcw, 1e-3, 200)                             # :176-351 (the per-step line is commented out, :293)
        if p.verbose and rinfo["iters"] >= 200:
            print("Max iterations reached")                                                   # :349
    finally:
        dprob.free()
    S_vec = S
    if perm is not None:
        S_vec = np.empty_like(S); S_vec[perm] = S
    if not return_info:
        return Rest, S_vec
    pos = lpinfo.pop("pos_edges")
    info = dict(lp=lpinfo, pos_edges=pos if perm is None else perm[pos], k=k, R_gcw=R_gcw, spectral=sinfo, refine=rinfo)
    if want_y:
        info["y"] = y
    return Rest, S_vec, info


def Rotation_Alignment(R_est, R_gt):
    """[R_out, R_align, mean_error, median_error] = Rotation_Alignment(R_est, R_gt)
    -- Utils/Rotation_Alignment.m:13-38 (evaluation helper: host NumPy, O(n))."""
    R_est = np.asarray(R_est, dtype=np.float64); R_gt = np.asarray(R_gt, dtype=np.float64)
    d, n = R_gt.shape[0], R_gt.shape[2]
    A = np.einsum("abk,ack->bc", R_est, R_gt)                 # sum_k R_est_k' R_gt_k
    U1, _, V1t = np.linalg.svd(A)
    D = np.eye(d); D[-1, -1] = np.linalg.det(U1 @ V1t)
    R_align = U1 @ D @ V1t
    R_out = np.einsum("abk,bc->ack", R_est, R_align)
    tr = np.einsum("abk,abk->k", R_gt, R_out)
    x = (tr - 1.0) / 2.0
    err = np.where(np.abs(x) <= 1, np.arccos(np.clip(x, -1, 1)), np.abs(np.arccos(x.astype(complex)))) / np.pi * 180
    return R_out, R_align, float(np.mean(err)), float(np.median(err))


def _alignment_blocks(x, b, name):
    """One entry of Rotation_Alignment_batch's lists as the 9 n doubles of its column-major 3x3xn blocks."""
    if name == "R_gt" and not isinstance(x, np.ndarray) and hasattr(x, "R_orig"):
        x = x.R_orig                                         # a model object
    try:
        x = np.asarray(x, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"problem {b}: {name} must be a 3x3xn array") from None
    if x.ndim != 3 or x.shape[0] != 3 or x.shape[1] != 3 or x.shape[2] < 1:
        raise ValueError(f"problem {b}: {name} must be 3x3xn with n >= 1, not of shape {x.shape}")
    flat = x.reshape(-1, order="F")                          # any memory order in, the ABI's out
    if not np.isfinite(flat).all():
        k = int(np.flatnonzero(~np.isfinite(flat))[0]) // 9
        raise ValueError(f"problem {b}: {name} of node {k + 1} is not finite")
    return flat


def Rotation_Alignment_batch(R_est_list, R_gt_list, rotations=True, device=0, return_info=False):
    """Rotation_Alignment (Utils/Rotation_Alignment.m:13-38) of many problems in one GPU pass: a list of the tuples (R_out, R_align,
    mean_error, median_error) Rotation_Alignment returns, one per problem.  R_out is Fortran-ordered 3x3xn, or None with
    ``rotations=False`` (it is three quarters of what comes back).  An entry of ``R_gt_list`` is a 3x3xn array or a model object, whose
    R_orig is used; arrays may be in any memory order.  With ``return_info`` every tuple gets a fifth member dict(err=..., timings=...),
    err the per-node errors in degrees.  Non-finite entries are refused: the nodes IRLS_GM leaves NaN outside the largest component must
    be masked by the caller.  Two empty lists give []."""
    for name, lst in (("R_est_list", R_est_list), ("R_gt_list", R_gt_list)):
        if isinstance(lst, (str, bytes, np.ndarray)) or not hasattr(lst, "__len__") or not hasattr(lst, "__getitem__"):
            raise ValueError(f"{name} must be a sequence of 3x3xn arrays")
    if len(R_est_list) != len(R_gt_list):
        raise ValueError(f"R_est_list holds {len(R_est_list)} problems, R_gt_list {len(R_gt_list)}")
    if not isinstance(device, (int, np.integer)) or isinstance(device, bool) or device < 0:
        raise ValueError("device must be a non-negative integer")
    est, gt = [], []
    for b, (e, g) in enumerate(zip(R_est_list, R_gt_list)):
        est.append(_alignment_blocks(e, b, "R_est"))
        gt.append(_alignment_blocks(g, b, "R_gt"))
        if est[-1].shape[0] != gt[-1].shape[0]:
            raise ValueError(f"problem {b}: R_est has n = {est[-1].shape[0] // 9}, R_gt n = {gt[-1].shape[0] // 9}")
    if not est:                                              # the empty batch touches no device
        return []
    if sum(x.shape[0] for x in gt) >= 2 ** 31:
        raise ValueError("the batch holds 2^31 / 9 nodes or more: split the batch")
    batch = _lib.AlignBatch([x.shape[0] // 9 for x in gt], np.concatenate(gt), device=int(device))
    try:
        out, timings = batch.run(np.concatenate(est), rotations=bool(rotations))
    finally:
        batch.destroy()
    R_out = _lib._split_R(out["R_out"], batch.node_off) if rotations else [None] * batch.count
    res = []
    for b in range(batch.count):
        n0, n1 = int(batch.node_off[b]), int(batch.node_off[b + 1])
        t = (R_out[b], out["R_align"][9 * b:9 * b + 9].reshape((3, 3), order="F"), float(out["mean_error"][b]), float(out["median_error"][b]))
        res.append(t + (dict(err=out["err"][n0:n1], timings=timings),) if return_info else t)
    return res

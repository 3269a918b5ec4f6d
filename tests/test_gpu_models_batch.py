"""GPU tests of the batched generators (csrc/models_batch.hip) against the NumPy restatement of their definition
(tests/models_batch_oracle.py): the draws, the graph pass at its wave and batch edges, the Nonuniform selections and their winner rule,
the rotations, ErrVec, independence of the batch's composition, and the hand-over to a batched solver."""
import numpy as np
import pytest

from tests import models_batch_cases as cases
from tests import models_batch_oracle as O

pytestmark = pytest.mark.gpu


def _stack(A):
    """3 x 3 x count (the library's layout) -> (count, 3, 3)."""
    return np.transpose(A, (2, 0, 1))


_drawn = {}


def drawn(kind, name):
    """The device's problems of a batch, drawn once and shared by the tests (treat as read-only)."""
    if (kind, name) not in _drawn:
        from desc_amd import Nonuniform_Topology_batch, Uniform_Topology_batch
        if kind == "uniform":
            _drawn[kind, name] = Uniform_Topology_batch(**cases.columns(cases.UNIFORM[name]))
        else:
            _drawn[kind, name] = Nonuniform_Topology_batch(**cases.columns(cases.NONUNIFORM[name]))
    return _drawn[kind, name]


ALL = [("uniform", k) for k in cases.UNIFORM] + [("nonuniform", k) for k in cases.NONUNIFORM]


def test_uniform_draws_are_bit_equal(lib):
    K = 2 ** 16
    for seed, stream, sub, id0, c in ((1, 1, 0, 0, 0), (2 ** 64 - 1, 8, 77, 2 ** 40, 3), (12345, 4, 0, 2 ** 31 - 5, 0)):
        got = lib.hook_models_draws(seed, stream, sub, id0, K, c)
        want = O.uniform(seed, stream, sub, np.arange(K, dtype=np.uint64) + np.uint64(id0), c)
        assert np.array_equal(got, want)
        assert got.min() >= 0.0 and got.max() < 1.0


def test_normal_draws(lib):
    K = 2 ** 16
    for seed, stream, sub, id0, c in ((1, 2, 0, 0, 0), (987654321, 9, 5, 2 ** 33, 8), (3, 5, 0, 100, 4)):
        got = lib.hook_models_draws(seed, stream, sub, id0, K, c, normal=True)
        want = O.normal(seed, stream, sub, np.arange(K, dtype=np.uint64) + np.uint64(id0), c)
        err = np.abs(got - want).max()
        print(f"normal draws (seed {seed}, stream {stream}): max |device - restated| = {err:.3e}")
        assert err <= 1e-13 and np.isfinite(got).all()


@pytest.mark.parametrize("kind,name", ALL)
def test_graph_and_flags_are_exact(lib, kind, name):
    assert lib.GUARD                                             # every buffer of the fetch was fenced and verified
    for b, (mo, ref) in enumerate(zip(drawn(kind, name), cases.restated(kind, name))):
        assert mo.n == ref.n and mo.seed == ref.seed
        assert mo.Ind.dtype == np.int64 and mo.Ind.shape == ref.Ind.shape and np.array_equal(mo.Ind, ref.Ind), (name, b)
        assert mo.corrupted.dtype == bool and np.array_equal(mo.corrupted, ref.corrupted), (name, b)
        m = ref.Ind.shape[0]
        for A, cnt in ((mo.RijMat, m), (mo.Rij_orig, m), (mo.R_orig, mo.n)):
            assert A.shape == (3, 3, cnt) and A.flags.f_contiguous and A.dtype == np.float64
        assert mo.ErrVec.shape == (m,)
        assert mo.AdjMat.shape == (mo.n, mo.n) and mo.AdjMat.sum() == 2 * m
    if (kind, name) == ("uniform", "complete"):
        assert [mo.Ind.shape[0] for mo in drawn(kind, name)] == [66, 65 * 64 // 2]
    if (kind, name) in (("uniform", "none"), ("uniform", "mixed")):
        assert any(mo.Ind.shape[0] == 0 for mo in drawn(kind, name))


@pytest.mark.parametrize("kind,name", ALL)
def test_rotations(kind, name):
    eye = np.eye(3)
    for b, (mo, ref) in enumerate(zip(drawn(kind, name), cases.restated(kind, name))):
        Ro, Rij, Rio = _stack(mo.R_orig), _stack(mo.RijMat), _stack(mo.Rij_orig)
        for R in (Ro, Rij, Rio):                                 # every block, the ill-conditioned ones included
            if R.shape[0]:
                assert np.abs(np.transpose(R, (0, 2, 1)) @ R - eye).max() <= 1e-13, (name, b)
                assert np.abs(np.linalg.det(R) - 1).max() <= 1e-13, (name, b)
        ii, jj = mo.Ind[:, 0] - 1, mo.Ind[:, 1] - 1
        if ii.size == 0:
            continue
        assert np.abs(Rio - Ro[ii] @ np.transpose(Ro[jj], (0, 2, 1))).max() <= 1e-14, (name, b)
        ok = ref.gap >= cases.GAP_MIN
        assert np.abs(Rij[ok] - ref.RijMat[ok]).max(initial=0) <= 1e-9, (name, b)
        assert np.abs(Rio[ok] - ref.Rij_orig[ok]).max(initial=0) <= 1e-9, (name, b)
        # a node's block: its own gap (an edge's gap includes its two nodes')
        _, gnode = O.project(O.normal_blocks(ref.seed, O.STREAM["rorig"], 0, np.arange(ref.n)))
        okn = gnode >= cases.GAP_MIN
        assert np.abs(Ro[okn] - ref.R_orig[okn]).max(initial=0) <= 1e-9, (name, b)


@pytest.mark.parametrize("kind,name", ALL)
def test_err_vec(kind, name):
    for b, (mo, ref) in enumerate(zip(drawn(kind, name), cases.restated(kind, name))):
        if mo.Ind.shape[0] == 0:
            continue
        tr = np.einsum("rck,rck->k", mo.Rij_orig, mo.RijMat)
        assert np.abs(np.cos(np.pi * mo.ErrVec) - (tr - 1) / 2).max() <= 1e-13, (name, b)
        assert (mo.ErrVec >= 0).all() and (mo.ErrVec <= 1 + 1e-7).all()
        ok = ref.gap >= cases.GAP_MIN
        assert np.abs(mo.ErrVec[ok] - ref.ErrVec[ok]).max(initial=0) <= 1e-7, (name, b)


def test_adv_blocks_show_winner_and_sign():
    """Under 'adv' with every edge selected from both ends, a wrong winner or a wrong sign of IndMat moves the block by O(1): the
    restated blocks are far from both alternatives, the device's are the restated ones."""
    for b, s in enumerate(cases.NONUNIFORM["all"]):
        if s["crpt_type"] != "adv":
            continue
        mo, ref = drawn("nonuniform", "all")[b], cases.restated("nonuniform", "all")[b]
        clean = O.nonuniform_topology(**{**s, "sigma_in": 0.0, "sigma_out": 0.0})
        assert np.array_equal(clean.winner, ref.winner) and ref.corrupted.all()
        # the other endpoint's block R_crpt_x R_orig_w' (transposed when x is the second node), and the right block transposed
        Rc, _ = O.project(O.normal_blocks(s["seed"], O.STREAM["rcorr"], 0, np.arange(s["n"])))
        ii, jj = ref.Ind[:, 0] - 1, ref.Ind[:, 1] - 1
        x = np.where(ref.winner == ii, jj, ii)
        Mx = Rc[x] @ np.transpose(ref.R_orig[ref.winner], (0, 2, 1))
        wrong_winner = np.where((x == ii)[:, None, None], Mx, np.transpose(Mx, (0, 2, 1)))
        wrong_sign = np.transpose(clean.RijMat, (0, 2, 1))
        for wrong in (wrong_winner, wrong_sign):
            assert np.median(np.abs(clean.RijMat - wrong).max(axis=(1, 2))) > 0.1
        ok = ref.gap >= cases.GAP_MIN
        assert np.abs(_stack(mo.RijMat)[ok] - ref.RijMat[ok]).max() <= 1e-9


def test_no_noise_no_corruption():
    from desc_amd import Nonuniform_Topology_batch, Uniform_Topology_batch
    mos = Uniform_Topology_batch([30, 65], 0.5, 0.0, 0.0, seeds=[5, 6]) + \
        Nonuniform_Topology_batch(30, 0.5, 0.0, 0.5, 0.0, 0.3, "adv", seeds=[7])
    for mo in mos:
        assert mo.Ind.shape[0] > 100 and not mo.corrupted.any()
        assert np.abs(mo.RijMat - mo.Rij_orig).max() <= 1e-14 and mo.ErrVec.max() <= 1e-7


def _same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("Ind", "RijMat", "Rij_orig", "R_orig", "ErrVec", "corrupted"))


def test_independence_of_the_batch():
    from desc_amd import Nonuniform_Topology_batch, Uniform_Topology_batch
    u = dict(n=40, p=0.5, q=0.3, sigma=0.1, model="self-consistent", seed=52)
    alone = Uniform_Topology_batch(**cases.columns([u]))[0]
    assert _same(alone, drawn("uniform", "mixed")[1])                               # inside the mixed batch, position 1
    other = [cases._uni(129, 0.4, 1), cases._uni(7, 1.0, 2), u, cases._uni(64, 0.2, 3)]
    again = Uniform_Topology_batch(**cases.columns(other))
    assert _same(alone, again[2])                                                   # another batch, another position
    assert _same(alone, Uniform_Topology_batch(**cases.columns([u, u]))[1])         # the same seed twice
    assert not np.array_equal(alone.Ind, Uniform_Topology_batch(**cases.columns([dict(u, seed=53)]))[0].Ind)
    v = cases.NONUNIFORM["partial"][0]
    alone = Nonuniform_Topology_batch(**cases.columns([v]))[0]
    assert _same(alone, drawn("nonuniform", "partial")[0])
    mixed = Nonuniform_Topology_batch(**cases.columns([cases.NONUNIFORM["all"][4], cases.NONUNIFORM["partial"][2], v]))
    assert _same(alone, mixed[2])


def test_return_info():
    from desc_amd import Uniform_Topology_batch
    mos, tm = Uniform_Topology_batch(40, 0.5, 0.3, 0.1, seeds=[1, 2, 3], return_info=True)
    assert len(mos) == 3 and set(tm) == {"ms_graph", "ms_nodes", "ms_edges", "ms_copy", "ms_total"}
    assert all(tm[k] > 0 for k in tm) and tm["ms_total"] >= tm["ms_graph"] + tm["ms_nodes"] + tm["ms_edges"]


def test_generated_models_go_through_a_batched_solver():
    from desc_amd import ConstantStepSize, DESC_PGD_batch, Uniform_Topology_batch
    mos = Uniform_Topology_batch(30, 0.6, 0.3, 0.05, seeds=[11, 12, 13])
    S = DESC_PGD_batch(mos, dict(iters=20, Gradient=ConstantStepSize(0.01), seed=1, verbose=False))
    for mo, s in zip(mos, S):
        assert s.shape == mo.ErrVec.shape and np.isfinite(s).all()
        assert mo.corrupted.any() and not mo.corrupted.all()
        assert s[mo.corrupted].mean() > s[~mo.corrupted].mean()

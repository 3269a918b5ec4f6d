"""CPU tests (no GPU) of the batched generators (desc_models_batch_*, Uniform_Topology_batch, Nonuniform_Topology_batch): ABI surface,
the refusals that come before any device call, the key of the NumPy restatement against the library's, the restatement's
hand-checkable cases and its distributions."""
import ctypes as C

import numpy as np
import pytest

from tests import models_batch_cases as cases
from tests import models_batch_oracle as O

SYMBOLS = ["desc_models_key", "desc_models_batch_max_n", "desc_models_batch_create", "desc_models_batch_sizes", "desc_models_batch_fetch",
           "desc_models_batch_destroy", "desc_test_models_uniform", "desc_test_models_normal"]


def test_abi_surface(lib):
    import desc_amd
    L = lib.load()
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/desc_amd.h").read()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS and name + "(" in hdr, name
    assert C.sizeof(lib.ModelSpec) == 80 and C.sizeof(lib.ModelsBatchTimings) == 40          # as include/desc_amd.h states
    for name in ("Uniform_Topology_batch", "Nonuniform_Topology_batch"):
        assert callable(getattr(desc_amd, name)) and name in desc_amd.__all__
    cap = lib.models_batch_max_n()
    assert cap >= 10000 and cap * (cap - 1) // 2 < 2 ** 31                                  # a problem's edge ids are int32
    for name, code in O.STREAM.items():
        assert lib.MODELS_STREAMS[name] == code and f"DESC_MODELS_STREAM_{name.upper()}" in hdr


def test_python_refusals_come_before_any_device_call(lib, monkeypatch):
    from desc_amd import Nonuniform_Topology_batch, Uniform_Topology_batch

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(lib, "ModelsBatch", no_device)
    cap = lib.models_batch_max_n()
    U = lambda **kw: Uniform_Topology_batch(**{**dict(n=10, p=0.5, q=0.2, sigma=0.1, seeds=[1, 2]), **kw})
    N = lambda **kw: Nonuniform_Topology_batch(**{**dict(n=10, p=0.5, p_node_crpt=0.2, p_edge_crpt=0.5, sigma_in=0.1, sigma_out=0.2, seeds=[1, 2]), **kw})
    for call in (U, N):
        with pytest.raises(ValueError, match="problem 1: n = 1, need n >= 2"):
            call(n=[10, 1])
        with pytest.raises(ValueError, match=f"problem 0: n = {cap + 1} exceeds {cap}"):
            call(n=cap + 1)
        with pytest.raises(ValueError, match="problem 0: n must be an integer"):
            call(n=10.5)
        for bad in (-0.1, 1.5, np.nan, np.inf):
            with pytest.raises(ValueError, match="problem 1: p must be a probability"):
                call(p=[0.5, bad])
        with pytest.raises(ValueError, match="one entry per problem \\(2\\), not 3"):
            call(p=[0.5, 0.5, 0.5])
        for bad in (None, 7, "ab", [[1, 2]]):
            with pytest.raises(ValueError, match="seeds must be a sequence"):
                call(seeds=bad)
        for bad in (-1, 2 ** 64, 1.5):
            with pytest.raises(ValueError, match="problem 1: the seed must be an integer"):
                call(seeds=[1, bad])
        with pytest.raises(ValueError, match="device"):
            call(device=-1)
        with pytest.raises(ValueError, match="2\\^30 edges or more at problem 1"):
            call(n=[10, cap], p=1.0)
        assert call(seeds=[]) == []
        assert call(seeds=[], return_info=True)[0] == []
    for bad in (-0.1, 1.5, np.nan):
        with pytest.raises(ValueError, match="problem 0: q must be a probability"):
            U(q=bad)
        with pytest.raises(ValueError, match="problem 0: p_node_crpt must be a probability"):
            N(p_node_crpt=bad)
        with pytest.raises(ValueError, match="problem 1: p_edge_crpt must be a probability"):
            N(p_edge_crpt=[0.5, bad])
    for bad in (-1e-3, np.nan, np.inf):
        with pytest.raises(ValueError, match="problem 0: sigma must be finite and >= 0"):
            U(sigma=bad)
        with pytest.raises(ValueError, match="problem 0: sigma_in must be finite and >= 0"):
            N(sigma_in=bad)
        with pytest.raises(ValueError, match="problem 1: sigma_out must be finite and >= 0"):
            N(sigma_out=[0.1, bad])
    with pytest.raises(ValueError, match="problem 1: unknown crpt_type 'haar'"):
        N(crpt_type=["adv", "haar"])
    with pytest.raises(ValueError, match="problem 0: model must be a string"):
        U(model=3)


def _spec(lib, **kw):
    base = dict(kind=lib.MODELS_KIND_UNIFORM, n=10, p=0.5, q=0.2, p_node_crpt=0.2, p_edge_crpt=0.5, sigma=0.1, sigma_in=0.1, sigma_out=0.2,
                mode=0, seed=1)
    return lib.ModelSpec(**{**base, **kw})


def test_c_entry_point_refuses_before_the_device(lib):
    """DESC_ERR_INVALID / DESC_ERR_TOO_LARGE naming the problem, and *out stays NULL.  Without a GPU a call that reached the device would
    return DESC_ERR_HIP instead; with one, the message is the same."""
    L = lib.load()
    cap = lib.models_batch_max_n()
    NU = lib.MODELS_KIND_NONUNIFORM
    bad = [(dict(n=1), "problem 1: n = 1, need n >= 2"), (dict(n=cap + 1), f"problem 1: n = {cap + 1} exceeds {cap}"),
           (dict(kind=2), "problem 1: unknown kind 2"), (dict(p=-0.1), "problem 1: p must be"), (dict(p=float("nan")), "problem 1: p must be"),
           (dict(q=1.1), "problem 1: q must be"), (dict(sigma=-1.0), "problem 1: sigma must be"), (dict(sigma=float("inf")), "problem 1: sigma must be"),
           (dict(kind=NU, p_node_crpt=2.0), "problem 1: p_node_crpt must be"), (dict(kind=NU, p_edge_crpt=float("nan")), "problem 1: p_edge_crpt must be"),
           (dict(kind=NU, sigma_in=-1.0), "problem 1: sigma_in must be"), (dict(kind=NU, sigma_out=float("nan")), "problem 1: sigma_out must be"),
           (dict(kind=NU, mode=3), "problem 1: unknown mode 3"), (dict(kind=NU, mode=-1), "problem 1: unknown mode -1")]
    for kw, text in bad:
        arr = (lib.ModelSpec * 2)(_spec(lib), _spec(lib, **kw))
        h = C.c_void_p(1)
        assert L.desc_models_batch_create(arr, 2, 0, C.byref(h)) == lib.ERR_INVALID and not h.value, kw
        assert text in L.desc_last_error().decode(), (kw, L.desc_last_error())
    h = C.c_void_p(1)
    assert L.desc_models_batch_create((lib.ModelSpec * 1)(_spec(lib)), -1, 0, C.byref(h)) == lib.ERR_INVALID and not h.value
    assert L.desc_models_batch_create(None, 1, 0, C.byref(h)) == lib.ERR_INVALID
    assert L.desc_models_batch_create((lib.ModelSpec * 1)(_spec(lib)), 1, 0, None) == lib.ERR_INVALID
    arr = (lib.ModelSpec * 2)(_spec(lib), _spec(lib, n=cap, p=1.0))
    h = C.c_void_p(1)
    assert L.desc_models_batch_create(arr, 2, 0, C.byref(h)) == lib.ERR_TOO_LARGE and not h.value
    assert "problem 1" in L.desc_last_error().decode()
    # a Uniform problem does not read the Nonuniform fields, a Nonuniform one not q and sigma, and any mode of a Uniform problem is
    # self-consistent: validation passes, and the call goes on to look for a device
    for kw in (dict(p_node_crpt=9.0, p_edge_crpt=-1.0, sigma_in=-1.0, sigma_out=float("nan"), mode=7), dict(kind=NU, q=9.0, sigma=-1.0)):
        h = C.c_void_p()
        rc = L.desc_models_batch_create((lib.ModelSpec * 1)(_spec(lib, **kw)), 1, 0, C.byref(h))
        assert rc in (lib.DESC_OK, lib.ERR_HIP), (kw, L.desc_last_error())
        if rc == lib.DESC_OK:
            L.desc_models_batch_destroy(h)
    # the draw hooks
    out = np.zeros(4)
    assert L.desc_test_models_uniform(1, 1, 0, 0, -1, 0, 0, lib.ptr(out, lib.F64P)) == lib.ERR_INVALID
    assert L.desc_test_models_normal(1, 1, 0, 0, 4, 0, 0, None) == lib.ERR_INVALID


def test_create_without_a_device_fails_with_err_hip(lib):
    if lib.load().desc_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(lib.DescError) as ei:
        lib.ModelsBatch([_spec(lib)])
    assert ei.value.code == lib.ERR_HIP
    h = C.c_void_p(1)
    assert lib.load().desc_models_batch_create((lib.ModelSpec * 1)(_spec(lib)), 1, 0, C.byref(h)) == lib.ERR_HIP and not h.value


def test_empty_batch_through_the_c_abi(lib):
    b = lib.ModelsBatch([])
    assert b.count == 0 and b.n == 0 and b.m == 0
    arrays, timings = b.fetch()
    assert all(v.size == 0 for v in arrays.values()) and timings["ms_nodes"] == 0
    b.destroy()


def test_restated_key_is_the_librarys(lib):
    L = lib.load()
    rng = np.random.default_rng(5)
    tri = rng.integers(0, 2 ** 64, size=(1000, 3), dtype=np.uint64)
    tri[:10] = [[0, 0, 0], [2 ** 64 - 1] * 3, [0, 2 ** 64 - 1, 0], [1, 0, 2 ** 64 - 1], [2 ** 63, 1, 1]] * 2
    want = np.array([L.desc_sample_key(int(a), int(b), int(c)) for a, b, c in tri], dtype=np.uint64)
    assert np.array_equal(O.sample_key(tri[:, 0], tri[:, 1], tri[:, 2]), want)
    assert int(O.mix64(0)[0]) == 0
    five = rng.integers(0, 2 ** 64, size=(200, 5), dtype=np.uint64)
    for s, st, sub, i, c in five:
        assert int(O.key(s, st, sub, [i], c)[0]) == lib.models_key(s, st, sub, i, c)
    # the draws' ranges, at the keys' extremes
    assert 0.0 <= O.uniform(1, 1, 0, np.arange(1000)).min() and O.uniform(1, 1, 0, np.arange(1000)).max() < 1.0
    assert (np.uint64(2 ** 64 - 1) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 < 1.0
    assert ((np.uint64(0) >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52 == 2.0 ** -53


def test_restatement_hand_checkable_cases():
    n = 9
    ii, jj = O.graph(n, 1.0, 3)
    want = [(i, j) for i in range(n) for j in range(i + 1, n)]
    assert list(zip(ii.tolist(), jj.tolist())) == want                                       # complete, sorted by (i, j)
    assert O.graph(n, 0.0, 3)[0].size == 0
    mo = O.uniform_topology(n, 0.0, 0.5, 0.1, seed=3)
    assert mo.Ind.shape == (0, 2) and mo.RijMat.shape == (0, 3, 3) and mo.ErrVec.shape == (0,) and mo.R_orig.shape == (n, 3, 3)
    assert not O.uniform_topology(n, 1.0, 0.0, 0.1, seed=3).corrupted.any()
    assert O.uniform_topology(n, 1.0, 1.0, 0.1, seed=3).corrupted.all()
    assert O.uniform_topology(n, 1.0, 1.0, 0.1, "self-consistent", seed=3).corrupted.all()
    clean = O.uniform_topology(n, 1.0, 0.0, 0.0, seed=3)
    assert np.abs(clean.RijMat - clean.Rij_orig).max() <= 1e-14 and clean.ErrVec.max() <= 1e-7
    assert O.corrupted_nodes(10, 0.25, 4).size == 2                                          # floor(2.5)
    assert O.corrupted_nodes(10, 0.0, 4).size == 0 and sorted(O.corrupted_nodes(10, 1.0, 4)) == list(range(10))
    # every edge selected by both ends: the endpoint later in the node order wins
    full = O.nonuniform_topology(10, 1.0, 1.0, 1.0, 0.0, 0.0, "adv", seed=4)
    pos = {int(v): r for r, v in enumerate(O.corrupted_nodes(10, 1.0, 4))}
    for (i, j), w in zip(full.Ind - 1, full.winner):
        assert w == (i if pos[i] > pos[j] else j)
    assert full.corrupted.all()
    # 'adv' without noise: the block is R_crpt_w R_orig_x' (transposed when w is the second node), far from the truth
    Rc, _ = O.project(O.normal_blocks(4, O.STREAM["rcorr"], 0, np.arange(10)))
    for k in (0, 17, 44):
        i, j = full.Ind[k] - 1
        w = full.winner[k]
        M = Rc[w] @ full.R_orig[j if w == i else i].T
        assert np.abs(full.RijMat[k] - (M if w == i else M.T)).max() <= 1e-13
    part = O.nonuniform_topology(10, 1.0, 0.25, 0.5, 0.0, 0.0, "uniform", seed=4)
    assert part.corrupted.sum() in (7, 8)                                                    # 2 nodes x floor(0.5 * 9) edges, one may be shared
    assert not O.nonuniform_topology(10, 1.0, 1.0, 0.0, 0.1, 0.1, seed=4).corrupted.any()


def test_restatement_distributions():
    """Fixed seeds, bounds six standard errors wide."""
    n, p, q = 300, 0.3, 0.25
    pairs = n * (n - 1) // 2
    mo = O.uniform_topology(n, p, q, 0.1, seed=12345)
    m = mo.Ind.shape[0]
    assert abs(m - pairs * p) <= 6 * np.sqrt(pairs * p * (1 - p))
    assert abs(mo.corrupted.mean() - q) <= 6 * np.sqrt(q * (1 - q) / m)
    # Haar blocks: E trace = 0, E trace^2 = 1 (the character of the defining representation); Var(trace) = 1 and
    # Var(trace^2) = E trace^4 - 1 = 3 - 1 = 2 (trace^4's mean counts the trivial summands of the fourfold tensor power: 3)
    K = 40000
    R, _ = O.project(O.normal_blocks(99, O.STREAM["haar"], 0, np.arange(K)))
    assert np.abs(np.linalg.det(R) - 1).max() <= 1e-12
    tr = np.trace(R, axis1=1, axis2=2)
    assert abs(tr.mean()) <= 6 * np.sqrt(1.0 / K)
    assert abs((tr ** 2).mean() - 1.0) <= 6 * np.sqrt(2.0 / K)
    # the normals themselves: mean 0, variance 1 (Var z^2 = 2)
    z = O.normal(7, O.STREAM["noise"], 0, np.arange(200000), 4)
    assert abs(z.mean()) <= 6 / np.sqrt(z.size) and abs((z ** 2).mean() - 1) <= 6 * np.sqrt(2.0 / z.size)
    # corrupted edges of the 'uniform' model: the Haar angle has density (1 - cos t) / pi on [0, pi]: mean pi/2 + 2/pi, second
    # moment pi^2/3 + 2, so ErrVec = t / pi has mean 1/2 + 2/pi^2 and variance 1/3 + 2/pi^2 - (1/2 + 2/pi^2)^2
    ev = mo.ErrVec[mo.corrupted]
    mean = 0.5 + 2 / np.pi ** 2
    var = 1.0 / 3 + 2 / np.pi ** 2 - mean ** 2
    assert ev.size > 2000 and abs(ev.mean() - mean) <= 6 * np.sqrt(var / ev.size)


def test_the_gpu_tests_batches_are_well_conditioned():
    """What tests/test_gpu_models_batch.py leaves out of its comparison with LAPACK's SVD is at most 0.1 % of a batch's blocks."""
    for kind, table in (("uniform", cases.UNIFORM), ("nonuniform", cases.NONUNIFORM)):
        for name in table:
            gaps = np.concatenate([mo.gap for mo in cases.restated(kind, name)])
            if gaps.size:
                assert (gaps < cases.GAP_MIN).mean() <= 1e-3, (kind, name)

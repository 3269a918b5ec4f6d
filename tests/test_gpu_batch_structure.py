"""GPU tests of the batched device structure builder (desc_pgd_batch_create_where with DESC_BUILD_DEVICE, build="device"): the
index arrays it makes against the oracle's structure of every problem ALONE and, with everything downstream of them, bit for bit
against the host builder's batch of the same problems."""
import numpy as np
import pytest

from desc_amd.algorithms import marshal_edges
from tests import batch_cap_cases as cases
from tests import graph_shapes as gs
from tests.helpers import STRUCT_KEYS, assert_structure_equal, c_params
from tests.test_gpu_batch import MIXED, path_graph, uniform

pytestmark = pytest.mark.gpu
SEED = 1
SEEDS = [7, 1, 123456789012, 0, 5]
RUN_KEYS = ("S_vec", "w", "obj", "avg")


def arrays(lib, q):
    return lib.ProblemArrays(q["n"], q["ii"], q["jj"], q["rij"])


def run(lib, probs, p, where, seeds=None, structures=True):
    """(structures, s0, outs, built_where) of one batch."""
    b = lib.Batch([arrays(lib, q) for q in probs], p, seeds, where)
    try:
        s0 = b.s0()
        outs, _ = b.run(p, want_w=True)
        sts = [b.structure(k) for k in range(b.count)] if structures else None      # after the run: the plain run needs no download
        return sts, s0, outs, b.built_where
    finally:
        b.destroy()


def same_structure(a, b):
    assert_structure_equal(a, b)
    assert (a["n"], a["m"], a["max_cnt"]) == (b["n"], b["m"], b["max_cnt"]) and np.array_equal(a["codeg"], b["codeg"])


def same_run(a, b):
    """equal_nan: average_change of a problem without an edge is 0 / 0 under either builder."""
    for key in RUN_KEYS:
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert a["iters_run"] == b["iters_run"] and a["n_sample"] == b["n_sample"]


def both_builders(lib, probs, p, seeds=None):
    """The batch under both builders: equal structures, S0 and run bits per problem.  Returns the device side."""
    dev = run(lib, probs, p, lib.BUILD_DEVICE, seeds)
    host = run(lib, probs, p, lib.BUILD_HOST, seeds)
    assert dev[3] == lib.BUILD_DEVICE and host[3] == lib.BUILD_HOST
    for k in range(len(probs)):
        same_structure(dev[0][k], host[0][k])
        assert np.array_equal(dev[1][k], host[1][k])
        same_run(dev[2][k], host[2][k])
    return dev


def rotations(m, seed):
    """m random rotations as m x 9 blocks."""
    rng = np.random.default_rng(seed)
    Q, R = np.linalg.qr(rng.standard_normal((m, 3, 3)))
    Q = Q * np.sign(np.einsum("kii->ki", R))[:, None, :]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]
    return np.ascontiguousarray(Q.reshape(m, 9))


def complete(n, seed=3):
    ii, jj = np.triu_indices(n, 1)
    return dict(mo=None, n=n, ii=ii.astype(np.int32), jj=jj.astype(np.int32), rij=rotations(ii.size, seed))


def from_model(mo):
    n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None
    return dict(mo=mo, n=n, ii=ii, jj=jj, rij=rij)


@pytest.fixture(scope="module")
def mixed():
    return [uniform(n, p, s) for n, p, s in MIXED]


@pytest.fixture(scope="module")
def mixed_dev(lib, mixed):
    """The MIXED batch with per-problem seeds under the device builder, once."""
    return run(lib, mixed, c_params(30, lr=0.01, seed=99), lib.BUILD_DEVICE, SEEDS)


def test_mixed_batch_against_oracle_and_host_builder(lib, oracle, mixed, mixed_dev):
    """Lane groups of 16, 32 and 64, n_sample = 34 for the fourth problem, per-problem seeds."""
    sts, s0, outs, built = mixed_dev
    assert built == lib.BUILD_DEVICE
    for q, sd, st in zip(mixed, SEEDS, sts):
        ref = oracle.build_structure(q["n"], q["ii"], q["jj"], seed=sd)
        assert_structure_equal(st, ref)
        assert np.array_equal(st["codeg"], ref["codeg"])
    assert sts[3]["n_sample"] == 34
    hsts, hs0, houts, hbuilt = run(lib, mixed, c_params(30, lr=0.01, seed=99), lib.BUILD_HOST, SEEDS)
    assert hbuilt == lib.BUILD_HOST
    for k in range(len(mixed)):
        same_structure(sts[k], hsts[k])
        assert np.array_equal(s0[k], hs0[k])
        same_run(outs[k], houts[k])


def test_composition_independence(lib, mixed, mixed_dev):
    """The batch as given, reversed, and every problem as a batch of one: the same structure arrays and result bits per problem."""
    sts, s0, outs, _ = mixed_dev
    p = c_params(30, lr=0.01, seed=99)
    B = len(mixed)
    rsts, rs0, routs, _ = run(lib, mixed[::-1], p, lib.BUILD_DEVICE, SEEDS[::-1])
    for k in range(B):
        same_structure(sts[k], rsts[B - 1 - k])
        assert np.array_equal(s0[k], rs0[B - 1 - k])
        same_run(outs[k], routs[B - 1 - k])
        asts, as0, aouts, built = run(lib, [mixed[k]], p, lib.BUILD_DEVICE, [SEEDS[k]])
        assert built == lib.BUILD_DEVICE
        same_structure(sts[k], asts[0])
        assert np.array_equal(s0[k], as0[0])
        same_run(outs[k], aouts[0])


def test_exact_selection_gives_the_same_structures(lib, mixed, mixed_dev, monkeypatch):
    """DESC_DEBUG_EXACT_SELECT=1: the tie-safe ranking for every sampled edge."""
    monkeypatch.setenv("DESC_DEBUG_EXACT_SELECT", "1")
    sts, s0, outs, built = run(lib, mixed, c_params(30, lr=0.01, seed=99), lib.BUILD_DEVICE, SEEDS)
    assert built == lib.BUILD_DEVICE
    for k in range(len(mixed)):
        same_structure(sts[k], mixed_dev[0][k])
        same_run(outs[k], mixed_dev[2][k])


@pytest.mark.parametrize("where_path", ["first", "middle", "last", "only"])
def test_triangle_free_problems(lib, oracle, where_path):
    """path_graph(8) has no 3-cycle: no segment, no cycle, S_vec = 1.  First, in the middle, last, and a batch of nothing else."""
    a, b = uniform(40, 0.5, 10), uniform(12, 0.6, 9)
    probs = {"first": [path_graph(8), a, b], "middle": [a, path_graph(8), b], "last": [a, b, path_graph(8)],
             "only": [path_graph(8), path_graph(5)]}[where_path]
    sts, s0, outs, _ = both_builders(lib, probs, c_params(20, lr=0.01, seed=SEED))
    for q, st, out in zip(probs, sts, outs):
        assert_structure_equal(st, oracle.build_structure(q["n"], q["ii"], q["jj"], seed=SEED))
        if q["mo"] is None:
            assert st["m_pos"] == 0 and st["m_cycle"] == 0 and np.array_equal(out["S_vec"], np.ones(q["n"] - 1)) and out["w"].size == 0


def test_sparse_graph_with_many_edges_without_a_cycle(lib, oracle):
    """Uniform_Topology(60, 0.08): a large share of the edges lies on no triangle, so pos_edge skips and the edge -> segment table
    holds -1 entries between used ones."""
    q = uniform(60, 0.08, 3)
    ref = oracle.build_structure(q["n"], q["ii"], q["jj"], seed=SEED)
    assert 0 < ref["m_pos"] < 0.8 * q["ii"].size
    probs = [uniform(12, 0.6, 9), q, uniform(40, 0.5, 10)]
    sts, _, _, _ = both_builders(lib, probs, c_params(20, lr=0.01, seed=SEED))
    assert_structure_equal(sts[1], ref)


def test_complete_graphs_around_n_sample(lib, oracle):
    """K31 (codegree 29: nothing sampled), K32 (30 = n_sample: the sampling branch with nothing to drop) and K33 (30 of 31)."""
    probs = [complete(31), complete(32), complete(33)]
    sts, _, _, _ = both_builders(lib, probs, c_params(10, lr=0.01, seed=SEED))
    for q, st, cnt in zip(probs, sts, (29, 30, 30)):
        assert_structure_equal(st, oracle.build_structure(q["n"], q["ii"], q["jj"], seed=SEED))
        assert st["n_sample"] == 30 and set(np.diff(st["cum_ind"]).tolist()) == {cnt}
    assert (sts[2]["ikj"] < 0).any()                          # K33 drops cycles, so some mirror cycles are not sampled


def test_rows_and_codegrees_above_one_wave(lib, oracle):
    """(150, 0.95, 6): CSR rows of ~142 entries and codegrees of ~135, so the intersection and the key passes loop over the wave."""
    q = uniform(150, 0.95, 6)
    ref = oracle.build_structure(q["n"], q["ii"], q["jj"], seed=SEED)
    assert ref["codeg"].min() > 64
    sts, _, _, _ = both_builders(lib, [q], c_params(10, lr=0.01, seed=SEED))
    assert_structure_equal(sts[0], ref)


def test_k258_is_accepted_with_full_wave_segments(lib, oracle):
    """K258: every codegree 256, n_sample = 64: segments of 64 cycles, lane groups of 64."""
    q = complete(258)
    sts, _, outs, _ = both_builders(lib, [q], c_params(3, lr=0.01, seed=SEED))
    assert sts[0]["n_sample"] == 64 and sts[0]["max_cnt"] == 64 and set(np.diff(sts[0]["cum_ind"]).tolist()) == {64}
    assert_structure_equal(sts[0], oracle.build_structure(q["n"], q["ii"], q["jj"], seed=SEED))


def _refusal(lib, probs, where, p=None):
    with pytest.raises(lib.DescError) as ei:
        lib.Batch([arrays(lib, q) for q in probs], p or c_params(5, seed=SEED), None, where)
    return ei.value.code, str(ei.value).split(": ", 1)[-1]


@pytest.mark.parametrize("place", ["alone", "third"])
def test_k259_is_refused_alike_and_the_handle_is_released(lib, place):
    """K259 has n_sample = 65.  The device builder knows only after its read-back; it closes the handle, and the next create works."""
    a, b = uniform(12, 0.6, 9), uniform(40, 0.5, 10)
    probs = [complete(259)] if place == "alone" else [a, b, complete(259)]
    name = "problem %d" % (len(probs) - 1)
    code_h, msg_h = _refusal(lib, probs, lib.BUILD_HOST)
    code_d, msg_d = _refusal(lib, probs, lib.BUILD_DEVICE)
    assert code_h == code_d == lib.ERR_INVALID and name in msg_h and name in msg_d and "n_sample = 65" in msg_d
    assert msg_h == msg_d
    both_builders(lib, [a, b], c_params(5, lr=0.01, seed=SEED))


def test_an_edge_listed_twice_is_refused_alike(lib):
    a, b = uniform(12, 0.6, 9), uniform(40, 0.5, 10)
    twice = dict(b, ii=np.concatenate([b["ii"][:5], b["ii"][4:]]), jj=np.concatenate([b["jj"][:5], b["jj"][4:]]),
                 rij=np.concatenate([b["rij"].reshape(-1, 9)[:5], b["rij"].reshape(-1, 9)[4:]]))
    got = [_refusal(lib, [a, twice], w) for w in (lib.BUILD_HOST, lib.BUILD_DEVICE)]
    assert got[0] == got[1] and got[0][0] == lib.ERR_INVALID and "problem 1" in got[0][1]


@pytest.mark.parametrize("place", ["alone", "second"])
def test_an_empty_edge_list_is_treated_alike(lib, place):
    """A problem without an edge: whatever the host builder does with it, the device builder does the same."""
    empty = dict(mo=None, n=5, ii=np.zeros(0, np.int32), jj=np.zeros(0, np.int32), rij=np.zeros(0))
    probs = [empty] if place == "alone" else [uniform(12, 0.6, 9), empty, uniform(40, 0.5, 10)]
    p = c_params(5, lr=0.01, seed=SEED)
    try:
        host = run(lib, probs, p, lib.BUILD_HOST)
    except lib.DescError as e:
        code_d, msg_d = _refusal(lib, probs, lib.BUILD_DEVICE, p)
        assert (code_d, msg_d) == (e.code, str(e).split(": ", 1)[-1])
        return
    dev = run(lib, probs, p, lib.BUILD_DEVICE)
    assert dev[3] == lib.BUILD_DEVICE
    for k in range(len(probs)):
        same_structure(dev[0][k], host[0][k])
        assert np.array_equal(dev[1][k], host[1][k])
        same_run(dev[2][k], host[2][k])


def test_row_above_the_cap_falls_back_and_the_cap_itself_does_not(lib):
    """A hub adjacent to everyone (tests/batch_cap_cases.py: row_cap): with cap + 1 neighbours the whole batch is built on the host,
    silently, with the host batch's results; with exactly cap neighbours it stays on the device."""
    cap = lib.cemp_batch_max_degree()
    small = uniform(12, 0.6, 9)
    p = c_params(5, lr=0.01, seed=SEED)
    at_cap = from_model(cases.row_cap(2000))
    assert np.bincount(np.concatenate([at_cap["ii"], at_cap["jj"]])).max() == cap
    both_builders(lib, [small, at_cap], p)
    over = from_model(gs.hub(cap + 2, 0.002, [2000], q=0.0, sigma=0.2, seed=72))
    assert np.bincount(np.concatenate([over["ii"], over["jj"]])).max() == cap + 1
    fell = run(lib, [small, over], p, lib.BUILD_DEVICE)
    host = run(lib, [small, over], p, lib.BUILD_HOST)
    assert fell[3] == lib.BUILD_HOST
    for k in range(2):
        same_structure(fell[0][k], host[0][k])
        assert np.array_equal(fell[1][k], host[1][k])
        same_run(fell[2][k], host[2][k])


def test_codegree_above_the_cap_falls_back_and_the_cap_itself_does_not(lib):
    """desc_pgd_batch_max_codeg() is reachable with n_sample <= 64: in gs.book(pages) the spine has codegree ``pages`` and the 2 pages
    other edges codegree 1, so the median is 1 and n_sample = 30.  pages = cap: the spine's 1024 common neighbours are staged and 30
    kept; pages = cap + 1: known after the read-back, the device half is closed and the batch is built on the host."""
    cap = lib.pgd_batch_max_codeg()
    small = uniform(12, 0.6, 9)
    p = c_params(5, lr=0.01, seed=SEED)
    at_cap = from_model(gs.book(cap, seed=5))
    sts, _, _, _ = both_builders(lib, [at_cap, small], p)
    assert sts[0]["codeg"].max() == cap and sts[0]["n_sample"] == 30 and np.diff(sts[0]["cum_ind"]).max() == 30
    over = from_model(gs.book(cap + 1, seed=5))
    fell = run(lib, [over, small], p, lib.BUILD_DEVICE)
    host = run(lib, [over, small], p, lib.BUILD_HOST)
    assert fell[3] == lib.BUILD_HOST and fell[0][0]["codeg"].max() == cap + 1
    for k in range(2):
        same_structure(fell[0][k], host[0][k])
        same_run(fell[2][k], host[2][k])
    both_builders(lib, [small], p)                            # the closed device half left nothing behind


def test_python_layer(lib):
    """DESC_PGD_batch, DESC_init_batch and DESC_batch on six 40-node problems with an unsorted Ind: build="device" gives the bits of
    build="host"; the info dicts say which builder ran."""
    from desc_amd import ConstantStepSize, DESC_batch, DESC_init_batch, DESC_PGD_batch
    probs = []
    for s in range(6):
        mo = uniform(40, 0.5, 20 + s)["mo"]
        perm = np.random.default_rng(s).permutation(mo.Ind.shape[0])
        probs.append((mo.Ind[perm], mo.RijMat[:, :, perm]))
    par = lambda: dict(iters=20, Gradient=ConstantStepSize(0.01), seed=SEED, verbose=False)
    S_h, S_d = DESC_PGD_batch(probs, par()), DESC_PGD_batch(probs, par(), build="device")
    info = DESC_PGD_batch(probs, par(), return_info=True, build="device")
    info_h = DESC_PGD_batch(probs, par(), return_info=True)
    for k in range(6):
        assert np.array_equal(S_h[k], S_d[k]) and np.array_equal(info[k]["S_vec"], S_h[k]) and np.array_equal(info[k]["w"], info_h[k]["w"])
        assert info[k]["built_where"] == "device" and info_h[k]["built_where"] == "host"
    init_h, init_d = DESC_init_batch(probs, par(), return_info=True), DESC_init_batch(probs, par(), return_info=True, build="device")
    for (R_h, Sh, ih), (R_d, Sd, idd) in zip(init_h, init_d):
        assert np.array_equal(R_h, R_d) and np.array_equal(Sh, Sd)
        assert ih["pgd"]["built_where"] == "host" and idd["pgd"]["built_where"] == "device"
    full_h, full_d = DESC_batch(probs, par(), return_info=True), DESC_batch(probs, par(), return_info=True, build="device")
    for (Re_h, Ri_h, Sh, ih), (Re_d, Ri_d, Sd, idd) in zip(full_h, full_d):
        assert np.array_equal(Re_h, Re_d) and np.array_equal(Ri_h, Ri_d) and np.array_equal(Sh, Sd)
        assert ih["pgd"]["built_where"] == "host" and idd["pgd"]["built_where"] == "device"
    lib.verify_guards()

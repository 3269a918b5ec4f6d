"""GPU tests of the CEMP, MST, MPLS and IRLS calls on a resident problem set (desc_cemp_batch_create_on, desc_irls_batch_create_on,
desc_mst_batch_run_on; desc_mpls_batch_run on a handle created on a set).  Every comparison is exact: each call on the set against the
same call on the list, bit for bit.  The byte counters are conditions derived from the record sizes, not measurements.

The shapes sit at the edges of the small kernels behind a create_on, not at the workload's: four problems of different sizes (nonzero
offsets), m < 256 and m > 256 (the strided edge -> problem and order loops), a sparse band of 262 nodes (the sign kernel's row loop and
the tree gather's 261 slots stride more than once), a hub of degree 69 (a row longer than a wave), one problem with permuted edge rows
(the non-identity order upload; tree_edges and SVec come back in the caller's rows)."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import graph_shapes as gs
from tests.helpers import make_problem
from tests.test_gpu_problem_batch import same

pytestmark = pytest.mark.gpu

CEMP = dict(max_iter=2, reweighting=[1.0, 2.0], nsample=5, seed=1)
MPLS = dict(stop_threshold=1e-3, max_iter=2, reweighting=[1.0, 2.0], thresholding=[0.95, 0.9], cycle_info_ratio=[1.0, 0.9])
IRLS = dict(MaxIterations=(1, 2))
CALLS = ("cemp", "cemp_gcw", "mst", "cemp_mst", "mpls", "irls_gm", "irls_l12")


def _shapes():
    small = make_problem("uniform", n=12, p=0.7, seed=1)[0]                                  # m < 256
    mid = make_problem("uniform", n=33, p=0.4, seed=2)[0]
    perm = np.random.default_rng(5).permutation(mid.Ind.shape[0])
    mid = SimpleNamespace(Ind=mid.Ind[perm], RijMat=np.asfortranarray(mid.RijMat[:, :, perm]), ErrVec=mid.ErrVec[perm])
    sparse = gs.band(262, 2, seed=31, chords=[(1, 100), (50, 200), (3, 262), (120, 121 + 40)])      # n - 1 = 261 > 256, m > 256
    hub = gs.hub(70, 0.1, [35], seed=32)                                                     # node 35 has 69 neighbours
    mos = [small, mid, sparse, hub]
    assert small.Ind.shape[0] < 256 < sparse.Ind.shape[0] and gs.degrees(hub.Ind).max() > 64 and gs.degrees(sparse.Ind).max() <= 6
    return mos


def _run_all(problems, mos, seeds):
    """The seven baseline calls on ``problems`` (a list or a ProblemBatch); ``mos`` gives the synthetic S_vec of MST_batch."""
    import desc_amd as D
    S = [gs.noisy_truth(mo, 7 + b) for b, mo in enumerate(mos)]
    return dict(cemp=D.CEMP_batch(problems, CEMP, seeds=seeds, return_info=True),
                cemp_gcw=D.CEMP_GCW_batch(problems, CEMP, seeds=seeds, return_info=True),
                mst=D.MST_batch(problems, S, return_info=True),
                cemp_mst=D.CEMP_MST_batch(problems, CEMP, seeds=seeds, return_info=True),
                mpls=D.MPLS_batch(problems, CEMP, MPLS, seeds=seeds, return_info=True),
                irls_gm=D.IRLS_GM_batch(problems, return_info=True, **IRLS),
                irls_l12=D.IRLS_L12_batch(problems, return_info=True, **IRLS))


@pytest.fixture(scope="module")
def on_list():
    mos = _shapes()
    return _run_all(mos, mos, [3, 4, 5, 6])


# ---- 1. bits on a built set

@pytest.mark.parametrize("csr", ["host", "device"])
def test_every_baseline_call_gives_the_lists_bits_on_a_built_set(on_list, csr):
    from desc_amd import ProblemBatch
    mos = _shapes()
    with ProblemBatch(mos, csr=csr) as ps:
        assert ps.built_where == csr and ps.perms[0] is None and ps.perms[1] is not None
        got = _run_all(ps, mos, [3, 4, 5, 6])
    assert tuple(got) == CALLS == tuple(on_list)
    for key in CALLS:
        assert same(on_list[key], got[key]), (csr, key)
    # the caller's rows: problem 1's SVec and tree edges follow its permuted Ind
    m1, n1 = mos[1].Ind.shape[0], int(mos[1].Ind.max())
    assert got["cemp"][1][0].shape == (m1,) and got["mst"][1][1]["tree_edges"].shape == (n1 - 1,)
    assert got["mst"][2][1]["tree_edges"].shape == (261,)


# ---- 2. bits on a generated set, 3a. no rotation comes down

GEN = dict(n=[12, 30, 65], p=0.7, q=0.2, sigma=0.1, model=["uniform", "self-consistent", "uniform"], seeds=[11, 12, 13])


def test_every_baseline_call_gives_the_lists_bits_on_a_generated_set_and_fetches_no_rotation():
    import desc_amd as D
    mos = D.Uniform_Topology_batch(**GEN)
    ps = D.Uniform_Topology_batch(**GEN, resident=True)
    M = sum(mo.Ind.shape[0] for mo in mos)
    moved = ps.bytes()
    assert moved[1] <= 8 * M + 64 * len(mos) < 72 * M                  # the endpoints came down, no rotation
    got = _run_all(ps, mos, [3, 4, 5])
    print(f"generated set: M = {M}, the set copied {moved} bytes (up, down) at creation and {ps.bytes()} after the seven calls")
    assert ps.bytes()[1] == moved[1]                                    # ... and none for any of the seven calls: this fails on the host mirror
    want = _run_all(mos, mos, [3, 4, 5])
    for key in CALLS:
        assert same(want[key], got[key]), key
    ps.close()


# ---- 3b. nothing large moves

def test_the_creates_and_the_tree_step_move_o_of_b_and_o_of_n_bytes(lib):
    """Bounds from the record sizes: CbProb is 32 bytes, MbProb 16, a tree sequence entry and an order entry 4, an S_vec entry 8, a tree
    block 72 and its edge id 4.  72 M (the rotations the list path uploads per handle) exceeds each bound tenfold; for the tree step's
    upload, whose 8 M bytes are the caller's S_vec and a ninth of 72 M by definition, that holds for what the call adds to its input."""
    from desc_amd.algorithms import _marshal_problems
    mos = [make_problem("uniform", n=40 + 3 * b, p=0.5, seed=30 + b)[0] for b in range(8)]
    probs, _ = _marshal_problems(mos)
    B, M, N = len(probs), sum(q.m for q in probs), sum(q.n for q in probs)
    bound = dict(cemp=256 * B, irls=4 * N + 256 * B, irls_perm=4 * N + 256 * B + 4 * M, mst_up_own=256 * B, mst_down=76 * N + 64 * B)
    for name, v in bound.items():
        assert 72 * M > 10 * v, (name, v, 72 * M)
    orders = [None] * B
    orders[3] = np.random.default_rng(1).permutation(probs[3].m).astype(np.int32)            # a row order that is not the identity
    with lib.ProblemBatch(probs, csr="device") as s:
        c = lib.CempBatch(None, 5, 0, list(range(B)), on=s)
        print(f"cemp: create_on moved {c.bytes()} bytes (bound {bound['cemp']} up, 0 down); a list-path create uploads >= {72 * M}")
        assert 0 < c.bytes()[0] <= bound["cemp"] and c.bytes()[1] == 0
        Sv = np.concatenate(c.run([1.0], 1)[0])
        mst, _, moved = lib.mst_batch_run_on(s, Sv, return_bytes=True)
        print(f"mst: run_on moved {moved} bytes (bounds {8 * M + 256 * B} up, {bound['mst_down']} down)")
        assert 8 * M <= moved[0] <= 8 * M + bound["mst_up_own"] and 72 * (N - B) <= moved[1] <= bound["mst_down"]
        R0 = np.concatenate([R.reshape(-1, order="F") for R, _ in mst])
        c.mpls_run(Sv, R0, 1e-3, 2, [1.0], [0.9], [1.0])                                     # the loop's setup: the signs by a launch
        assert c.bytes()[0] <= bound["cemp"] and c.bytes()[1] == 0
        i = lib.IrlsBatch(None, None, on=s)
        print(f"irls: create_on moved {i.bytes()} bytes (bound {bound['irls']} up, 0 down)")
        assert 0 < i.bytes()[0] <= bound["irls"] and i.bytes()[1] == 0
        ip = lib.IrlsBatch(None, orders, on=s)
        print(f"irls, one permuted order: create_on moved {ip.bytes()} bytes (bound {i.bytes()[0]} + {4 * M} up)")
        assert i.bytes()[0] < ip.bytes()[0] <= i.bytes()[0] + 4 * M and ip.bytes()[0] <= bound["irls_perm"] and ip.bytes()[1] == 0
        # the bytes are not all that is checked: the handles compute what list-path handles compute
        c0, i0 = lib.CempBatch(probs, 5, 0, list(range(B))), lib.IrlsBatch(probs, orders)
        assert same(c.run([1.0], 1)[0], c0.run([1.0], 1)[0]) and same(mst, lib.mst_batch_run(probs, Sv)[0])
        assert same(ip.run(lib.IRLS_GM, 5.0, 1, 1)[0], i0.run(lib.IRLS_GM, 5.0, 1, 1)[0])
        for h in (c, i, ip, c0, i0):
            h.destroy()


# ---- 4. lifetime

def test_cemp_and_irls_handles_outlive_the_set_and_run_twice(lib):
    from desc_amd.algorithms import _marshal_problems
    probs, perms = _marshal_problems(_shapes())
    seeds = [3, 4, 5, 6]
    s = lib.ProblemBatch(probs, csr="device")
    c, i = lib.CempBatch(None, 5, 1, seeds, on=s), lib.IrlsBatch(None, perms, on=s)         # two handles on one set, alive together
    s.close()                                                                                # ... and the set goes first
    assert not s.handle
    c0, i0 = lib.CempBatch(probs, 5, 1, seeds), lib.IrlsBatch(probs, perms)                  # fresh list-path handles
    Sv = c.run([1.0, 2.0], 2)[0]
    assert same(Sv, c0.run([1.0, 2.0], 2)[0]) and same(Sv, c.run([1.0, 2.0], 2)[0])          # run twice: the same bits
    Sv = np.concatenate(Sv)
    R0 = np.concatenate([R.reshape(-1, order="F") for R, _ in lib.mst_batch_run(probs, Sv)[0]])
    loop = (Sv, R0, 1e-3, 2, [1.0, 2.0], [0.95, 0.9], [1.0, 0.9])
    out = c.mpls_run(*loop)[0]                                                               # the loop's setup runs after the set was closed
    assert same(out, c0.mpls_run(*loop)[0]) and same(out, c.mpls_run(*loop)[0])
    for mode in (lib.IRLS_GM, lib.IRLS_L12):
        out = i.run(mode, 5.0, 1, 2)[0]
        assert same(out, i0.run(mode, 5.0, 1, 2)[0]) and same(out, i.run(mode, 5.0, 1, 2)[0])
    for h in (c, i, c0, i0):
        h.destroy()


# ---- 5. refusals on a set, in the list path's words

def _refusal(call):
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


def test_refusals_on_a_set_keep_the_lists_words():
    import desc_amd as D
    good, split = make_problem("uniform", n=12, p=0.7, seed=1)[0], gs.model("two_components")
    mos = [good, split]
    S = [np.full(mo.Ind.shape[0], 0.5) for mo in mos]
    ps = D.ProblemBatch(mos, csr="device")
    for call, words in ((lambda p: D.MST_batch(p, S), "problem 1: the graph is disconnected: 2 components"),
                        (lambda p: D.CEMP_MST_batch(p, CEMP), "problem 1: the graph is disconnected: 2 components"),
                        (lambda p: D.MPLS_batch(p, CEMP, MPLS), "problem 1: the graph is disconnected: 2 components"),
                        (lambda p: D.IRLS_GM_batch(p, **IRLS), "problem 1: the graph is not connected ("),
                        (lambda p: D.IRLS_L12_batch(p, **IRLS), "problem 1: the graph is not connected ("),
                        (lambda p: D.CEMP_batch(p, CEMP, seeds=[1]), "seeds must hold one entry per problem (2), not 1"),
                        (lambda p: D.MPLS_batch(p, CEMP, MPLS, seeds=[1, 2, 3]), "seeds must hold one entry per problem (2), not 3")):
        on_set = _refusal(lambda: call(ps))
        assert words in on_set and on_set == _refusal(lambda: call(mos)), words
    other = dict(CEMP, device=1)
    for call in (lambda: D.CEMP_batch(ps, other), lambda: D.CEMP_GCW_batch(ps, other), lambda: D.CEMP_MST_batch(ps, other),
                 lambda: D.MPLS_batch(ps, other, MPLS), lambda: D.MST_batch(ps, S, device=1), lambda: D.IRLS_GM_batch(ps, device=1, **IRLS),
                 lambda: D.IRLS_L12_batch(ps, device=1, **IRLS)):
        assert "device = 1 differs from the device of the ProblemBatch (0)" in _refusal(call)
    ps.close()
    for call in (lambda: D.CEMP_batch(ps, CEMP), lambda: D.CEMP_GCW_batch(ps, CEMP), lambda: D.CEMP_MST_batch(ps, CEMP),
                 lambda: D.MPLS_batch(ps, CEMP, MPLS), lambda: D.MST_batch(ps, S), lambda: D.IRLS_GM_batch(ps, **IRLS),
                 lambda: D.IRLS_L12_batch(ps, **IRLS)):
        assert "the ProblemBatch is closed" in _refusal(call)

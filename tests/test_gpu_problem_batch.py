"""GPU tests of the resident problem set (desc_problem_batch_*, the *_create_on calls, ProblemBatch, the generators' resident=True).
Every comparison is exact: the CSR kernel against the host builder element for element, every batched call on the set against the same
call on the list bit for bit, the generated set against the generated list field for field.  The byte counters are conditions: a
create_on uploads O(B) bytes, from_models copies down the endpoints and nothing else."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import graph_shapes as gs
from tests.helpers import make_problem

pytestmark = pytest.mark.gpu


def _pairs_problem(lib, pairs):
    """ProblemArrays of 0-based pairs (i < j), sorted, n = the largest endpoint + 1, distinct rotations about z."""
    P = np.unique(np.asarray(pairs, dtype=np.int32).reshape(-1, 2), axis=0)
    t = 0.1 * np.arange(1, P.shape[0] + 1)
    R = np.zeros((3, 3, P.shape[0]), order="F")
    R[0, 0], R[1, 1], R[0, 1], R[1, 0], R[2, 2] = np.cos(t), np.cos(t), -np.sin(t), np.sin(t), 1.0
    return lib.ProblemArrays(int(P.max()) + 1, P[:, 0], P[:, 1], R.reshape(-1, order="F"))


def _model_problem(lib, mo):
    from desc_amd.algorithms import marshal_edges
    n, ii, jj, rij, perm = marshal_edges(mo.Ind, mo.RijMat)
    assert perm is None
    return lib.ProblemArrays(n, ii, jj, rij)


def _complete(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def _star(n, hub=0):
    return [(min(hub, v), max(hub, v)) for v in range(n) if v != hub]


# name -> the problems of one set.  The named shapes are tests/graph_shapes.py's; the stars' rows of 65 and 257 cross a wave and a
# workgroup of the kernel; node 3 of "isolated_interior" touches no edge: an empty row between full ones.
CSR_CASES = {
    "hub_first": lambda lib: [_model_problem(lib, gs.model("hub600_first"))],
    "hub_middle": lambda lib: [_model_problem(lib, gs.model("hub300_mid"))],
    "hub_last": lambda lib: [_model_problem(lib, gs.model("hub600_last"))],
    "band": lambda lib: [_model_problem(lib, gs.model("band200_10"))],
    "star_first": lambda lib: [_model_problem(lib, gs.star(70, 1, seed=3))],
    "star_middle": lambda lib: [_model_problem(lib, gs.model("star200_mid"))],
    "star_last": lambda lib: [_model_problem(lib, gs.star(70, 70, seed=4))],
    "bipartite": lambda lib: [_model_problem(lib, gs.model("bipartite60_90"))],
    "bridged": lambda lib: [_model_problem(lib, gs.model("bridged150_60"))],
    "dense_with_pendants": lambda lib: [_model_problem(lib, gs.model("dense_pendants"))],
    "K2": lambda lib: [_pairs_problem(lib, [(0, 1)])],
    "K65": lambda lib: [_pairs_problem(lib, _complete(65))],
    "star66": lambda lib: [_pairs_problem(lib, _star(66))],
    "star258": lambda lib: [_pairs_problem(lib, _star(258))],
    "star258_hub_last": lambda lib: [_pairs_problem(lib, _star(258, 257))],
    "isolated_interior": lambda lib: [_pairs_problem(lib, [(0, 1), (0, 2), (1, 2), (1, 4), (2, 5), (4, 5), (0, 5)])],
    "mixed_2_66_7": lambda lib: [_pairs_problem(lib, [(0, 1)]), _pairs_problem(lib, _star(66, 30) + [(0, 65), (1, 2)]),
                                 _pairs_problem(lib, _complete(7))],
}


@pytest.mark.parametrize("name", list(CSR_CASES))
def test_csr_kernel_equals_the_host_builder(lib, name):
    probs = CSR_CASES[name](lib)
    small = all(q.n <= lib.gcw_batch_max_n() for q in probs)             # desc_gcw_batch_csr has the eigen-solve's cap
    want = lib.gcw_batch_csr(probs) if small else None                   # batch_csr_host through another door, no device
    got = {}
    for csr, where in (("host", lib.BUILD_HOST), ("device", lib.BUILD_DEVICE)):
        s = lib.ProblemBatch(probs, csr=csr)
        assert s.built_where == where and len(s) == len(probs)
        got[csr] = s.fetch(rij=True, csr=True)
        assert np.array_equal(s.node_off, np.concatenate([[0], np.cumsum([q.n for q in probs])]))
        assert np.array_equal(s.edge_off, np.concatenate([[0], np.cumsum([q.m for q in probs])]))
        s.close()
    if name == "isolated_interior":
        rp = got["host"]["rowptr"]
        assert rp[3] == rp[4] and rp[2] < rp[3] and rp[4] < rp[5]      # the empty row lies between rows that are not
    for key in ("ind_i", "ind_j", "rij", "rowptr", "adj", "adj_eid"):
        assert got["host"][key].shape == got["device"][key].shape and np.array_equal(got["host"][key], got["device"][key]), (name, key)
    assert np.array_equal(got["device"]["ind_i"], np.concatenate([q.ind_i for q in probs]))
    assert np.array_equal(got["device"]["ind_j"], np.concatenate([q.ind_j for q in probs]))
    assert np.array_equal(got["device"]["rij"], np.concatenate([q.rij for q in probs]))
    for key in ("rowptr", "adj", "adj_eid") if small else ():
        assert np.array_equal(got["device"][key], want[key]), (name, key)


# ---- the consumers: three problems of different n, the middle one with an unsorted Ind

PGD = dict(iters=25, verbose=False)
PGD_KEYS = ("S_vec", "iters_run", "obj_vals", "w", "n_sample", "average_change", "t_end", "built_where")


def _params():
    from desc_amd import ConstantStepSize
    return dict(PGD, Gradient=ConstantStepSize(0.01))


def _problems():
    mos = [make_problem("uniform", n=n, p=p, seed=seed)[0] for n, p, seed in ((12, 0.7, 1), (33, 0.4, 2), (20, 0.5, 3))]
    perm = np.random.default_rng(5).permutation(mos[1].Ind.shape[0])
    mos[1] = SimpleNamespace(Ind=mos[1].Ind[perm], RijMat=np.asfortranarray(mos[1].RijMat[:, :, perm]), ErrVec=mos[1].ErrVec[perm])
    return mos


def same(a, b):
    """Two results are the same in every bit; timings (``ms_*``, ``timings``) are not results."""
    if isinstance(a, dict):
        keys = [k for k in a if k != "timings" and not k.startswith("ms_")]
        return set(keys) == {k for k in b if k != "timings" and not k.startswith("ms_")} and all(same(a[k], b[k]) for k in keys)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def _run_all(problems):
    """Every call of the DESC row on ``problems`` (a list or a ProblemBatch)."""
    import desc_amd as D
    mos = _problems()
    S = [gs.noisy_truth(mo, 7 + b) for b, mo in enumerate(mos)]
    out = dict(spectral=D.Spectral_batch(problems, return_info=True), gcw=D.GCW_batch(problems, S, return_info=True))
    out["refine"] = D.DESC_refine_batch(problems, S, [R for R, _ in out["gcw"]], max_iters=6, return_info=True)
    for build in ("host", "device"):
        out["pgd_" + build] = D.DESC_PGD_batch(problems, _params(), seeds=[3, 4, 5], return_info=True, build=build)
    out["init"] = D.DESC_init_batch(problems, _params(), seeds=[3, 4, 5], return_info=True, build="device")
    out["desc"] = D.DESC_batch(problems, _params(), seeds=[3, 4, 5], return_info=True)
    return out


@pytest.fixture(scope="module")
def on_list():
    return _run_all(_problems())


@pytest.mark.parametrize("csr", ["host", "device"])
def test_every_desc_row_call_gives_the_lists_bits_on_the_set(on_list, csr):
    from desc_amd import ProblemBatch
    with ProblemBatch(_problems(), csr=csr) as ps:
        assert ps.built_where == csr and len(ps) == 3 and ps.perms[0] is None and ps.perms[1] is not None
        assert np.array_equal(ps[1].Ind, _problems()[1].Ind)
        got = _run_all(ps)
    assert set(got) == set(on_list)
    for key in on_list:
        assert same(on_list[key], got[key]), (csr, key)
    for build in ("host", "device"):
        for d in got["pgd_" + build]:
            assert d["built_where"] == build and all(k in d for k in PGD_KEYS)
    # the caller's edge order: problem 1's S_vec follows its unsorted Ind
    assert got["pgd_host"][1]["S_vec"].shape == (_problems()[1].Ind.shape[0],)


# ---- the generators

GEN = dict(uniform=dict(n=[12, 30, 65], p=0.7, q=0.2, sigma=0.1, model=["uniform", "self-consistent", "uniform"], seeds=[11, 12, 13]),
           nonuniform=dict(n=[12, 30, 65], p=0.7, p_node_crpt=0.3, p_edge_crpt=0.5, sigma_in=0.05, sigma_out=0.2,
                           crpt_type=["uniform", "self-consistent", "adv"], seeds=[21, 22, 23]))


@pytest.mark.parametrize("kind", list(GEN))
def test_resident_generator_equals_the_list(lib, kind):
    import desc_amd as D
    draw = D.Uniform_Topology_batch if kind == "uniform" else D.Nonuniform_Topology_batch
    mos = draw(**GEN[kind])
    ps = draw(**GEN[kind], resident=True)
    assert isinstance(ps, D.ProblemBatch) and len(ps) == len(mos) and ps.built_where == "device"
    M = sum(mo.Ind.shape[0] for mo in mos)
    up, down = ps.bytes()
    print(f"{kind}: M = {M}, from_models copied {up} bytes up, {down} bytes down (bound {8 * M + 64 * len(mos)})")
    assert down <= 8 * M + 64 * len(mos) and down < 72 * M              # the endpoints, no rotation
    desc = D.DESC_batch(ps, _params(), seeds=[3, 4, 5], build="device")
    assert ps.bytes()[1] == down                     # ... and none for the DESC row either
    want = D.DESC_batch(mos, _params(), seeds=[3, 4, 5], build="device")
    assert same(want, desc)
    ests = [R for R, _, _ in desc]
    assert same(D.Rotation_Alignment_batch(ests, mos), D.Rotation_Alignment_batch(ests, ps))
    for b, (mo, it) in enumerate(zip(mos, ps)):
        assert it.n == mo.n and it.seed == mo.seed
        for field in ("Ind", "ErrVec", "R_orig", "corrupted", "RijMat", "Rij_orig", "AdjMat"):
            x, y = getattr(mo, field), getattr(it, field)
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (kind, b, field)
    assert same(D.Spectral_batch(mos), D.Spectral_batch(ps))            # after the rotations were fetched, too
    ps.close()


def test_a_generated_problem_without_an_edge_is_refused():
    from desc_amd import Uniform_Topology_batch
    with pytest.raises(ValueError, match="problem 1: empty edge list"):
        Uniform_Topology_batch([12, 12, 12], [0.7, 0.0, 0.7], 0.2, 0.1, seeds=[1, 2, 3], resident=True)
    assert len(Uniform_Topology_batch([12, 12, 12], [0.7, 0.0, 0.7], 0.2, 0.1, seeds=[1, 2, 3])) == 3      # the list path takes it


# ---- lifetime

def test_handles_outlive_the_set_and_run_twice(lib):
    from desc_amd.algorithms import _marshal_problems
    probs, _ = _marshal_problems(_problems())
    S = np.concatenate([np.linspace(0.01, 0.9, q.m) for q in probs])
    s = lib.ProblemBatch(probs, csr="device")
    g, r = lib.GcwBatch(None, on=s), lib.RefineBatch(None, on=s)         # two handles on one set, alive together
    s.close()                                                            # ... and the set goes first
    assert not s.handle
    g0, r0 = lib.GcwBatch(probs), lib.RefineBatch(probs)                 # fresh list-path handles
    R = g.run(s_vec=S)[0]
    assert same(R, g0.run(s_vec=S)[0]) and same(R, g.run(s_vec=S)[0])    # run twice: the same bits
    R0 = np.concatenate([x.reshape(-1, order="F") for x, _ in R])
    out = r.run(S, R0, max_iters=5)[0]
    assert same(out, r0.run(S, R0, max_iters=5)[0]) and same(out, r.run(S, R0, max_iters=5)[0])
    for h in (g, r, g0, r0):
        h.destroy()


# ---- nothing large moves

def test_a_create_on_uploads_o_of_b_bytes(lib):
    """The device builder without fallback: what each create_on copies up is bounded by 256 bytes per problem, whatever the edges."""
    from desc_amd.algorithms import _marshal_problems
    mos = [make_problem("uniform", n=40 + 3 * b, p=0.5, seed=30 + b)[0] for b in range(8)]
    probs, _ = _marshal_problems(mos)
    B, M = len(probs), sum(q.m for q in probs)
    assert 72 * M > 100 * 256 * B                    # the rotations alone would be a hundred times the bound
    with lib.ProblemBatch(probs, csr="device") as s:
        handles = dict(gcw=lib.GcwBatch(None, on=s), refine=lib.RefineBatch(None, on=s),
                       pgd=lib.Batch(None, lib.default_params(), seeds=list(range(B)), where=lib.BUILD_DEVICE, on=s))
        assert handles["pgd"].built_where == lib.BUILD_DEVICE
        for name, h in handles.items():
            up, down = h.bytes()
            print(f"{name}: create_on uploaded {up} bytes (bound {256 * B}), the list-path create uploads >= {72 * M}")
            assert 0 <= up <= 256 * B and down == 0, name          # the eigen-solve borrows even its problem records: 0 bytes
        for h in handles.values():
            h.destroy()


# ---- the other families read the set's host mirror

def test_the_other_families_accept_the_set():
    import desc_amd as D
    mos = [make_problem("uniform", n=12, p=0.7, seed=40 + b)[0] for b in range(2)]
    cemp = dict(max_iter=1, reweighting=[1.0], nsample=5, seed=1)
    mpls = dict(stop_threshold=1e-3, max_iter=1, reweighting=[1.0], thresholding=[0.95], cycle_info_ratio=[1.0])
    calls = dict(cemp=lambda p: D.CEMP_batch(p, cemp), cemp_mst=lambda p: D.CEMP_MST_batch(p, cemp),
                 mpls=lambda p: D.MPLS_batch(p, cemp, mpls), irls_gm=lambda p: D.IRLS_GM_batch(p, MaxIterations=(1, 1)),
                 lp=lambda p: D.linprog_sij_batch(p, dict(max_iter=20, nsample=5), rotations=False))
    with D.ProblemBatch(mos) as ps:
        for name, call in calls.items():
            assert same(call(mos), call(ps)), name

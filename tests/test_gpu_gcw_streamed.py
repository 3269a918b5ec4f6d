"""GPU tests of the streamed eigen-solve (k_gcw_batch<true>, desc_gcw_batch_create_where, the ``eig`` keyword): the same bits as the
LDS kernel wherever both apply -- converged and at the unconverged exit --, problems above the LDS kernel's cap against the dense
LAPACK restatements, the bitwise independence of a problem's result from the batch and the mode around it, handle reuse, and the
four composite calls with eig="auto" on a batch that takes both kernels.  Tolerances as tests/test_gpu_gcw_batch.py: rotations
compared after rotation_alignment, max |R_aligned - R_ref| < 1e-8; |RR' - I| and |det - 1| < 1e-12."""
import numpy as np
import pytest

from desc_amd import ConstantStepSize, Rotation_Alignment
from desc_amd.algorithms import marshal_edges
from oracle.spectral_oracle import gcw_oracle, spectral_oracle
from tests import cemp_batch_cases
from tests import gcw_batch_cases as cases
from tests import gcw_streamed_cases as streamed
from tests import graph_shapes as gs
from tests.test_gpu_gcw_batch import aligned_diff, assert_rotations, same

pytestmark = pytest.mark.gpu

BIG = ("U279", "U400", "U748")


def arrays(lib, Ind, RijMat):
    n, ii, jj, rij, perm = marshal_edges(Ind, RijMat)
    assert perm is None
    return lib.ProblemArrays(n, ii, jj, rij)


def handle_run(lib, probs, eig, **run_args):
    h = lib.GcwBatch(probs, eig=eig)
    try:
        return h.run(**run_args)[0]
    finally:
        h.destroy()


# ---- 1. the same bits as the LDS kernel ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(lib):
    """Every size class of the LDS kernel's tests: 48 (v, c) items for 256 threads (n = 8) up to several strides of the staging copy and
    of the product (n = 278), rows == block width (the single edge), an empty CSR row."""
    mos = cases.mixed_models(lib.gcw_batch_max_n())
    S = list(cases.mixed_S(lib.gcw_batch_max_n()))
    edge = cases.single_edge()
    Ind, Rij, S_hole = cases.with_empty_row()
    probs = [arrays(lib, mo.Ind, mo.RijMat) for mo in mos] + [arrays(lib, edge.Ind, edge.RijMat), arrays(lib, Ind, Rij)]
    S = np.concatenate(S + [gs.noisy_truth(edge, 5), S_hole])
    assert [q.n for q in probs] == [8, 12, 40, 90, 150, 278, 10, 2, 20]
    return probs, S


@pytest.mark.parametrize("mode", ["gcw", "spectral", "weights"])
def test_streamed_equals_lds_bit_for_bit(lib, small, mode):
    probs, S = small
    args = dict(gcw=dict(s_vec=S), spectral=dict(), weights=dict(weights=1.0 / (S + 1e-8), normalize_rows=True))[mode]
    for max_iters in (500, 1, 3):                    # converged; the unconverged exit and its repeated Rayleigh-Ritz
        lds = handle_run(lib, probs, "lds", max_iters=max_iters, **args)
        got = handle_run(lib, probs, "streamed", max_iters=max_iters, **args)
        auto = handle_run(lib, probs, "auto", max_iters=max_iters, **args)
        print(mode, max_iters, [(i["iters"], i["products"], i["converged"]) for _, i in lds])
        for b, (x, y, z) in enumerate(zip(lds, got, auto)):
            assert same(x, y) and same(x, z), (mode, max_iters, b, x[1], y[1])
            assert (x[1]["eig"], y[1]["eig"], z[1]["eig"]) == ("lds", "streamed", "lds"), b
        conv = [i["converged"] for _, i in lds]
        if max_iters == 500:
            assert all(conv)
        else:
            if max_iters == 1:                       # only the single edge, whose start block spans the whole space, is done after one step
                assert conv == [False] * 7 + [True, False], conv
            assert all(i["iters"] == max_iters for (_, i), c in zip(lds, conv) if not c)


# ---- 2. above the LDS kernel's cap ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def above(lib):
    """[n = 40, U279, U400, U748] with eig="auto" in both modes, solved once; the dense oracle's and the single calls' answers."""
    from desc_amd import GCW, GCW_batch, Spectral, Spectral_batch
    mos = [cases.mixed_models(lib.gcw_batch_max_n())[2]] + [streamed.big(k)[0] for k in BIG]
    S = [cases.mixed_S(lib.gcw_batch_max_n())[2]] + [streamed.big(k)[1] for k in BIG]
    return dict(mos=mos, S=S, gcw=GCW_batch(mos, S, return_info=True, eig="auto"), spectral=Spectral_batch(mos, return_info=True, eig="auto"),
                gcw_ref=[gcw_oracle(mo.Ind, mo.RijMat, s) for mo, s in zip(mos, S)],
                spectral_ref=[spectral_oracle(mo.Ind, mo.RijMat) for mo in mos],
                gcw_single=[GCW(mo.Ind, None, mo.RijMat, s) for mo, s in zip(mos, S)],
                spectral_single=[Spectral(mo.Ind, mo.RijMat) for mo in mos])


@pytest.mark.parametrize("mode", ["gcw", "spectral"])
def test_above_the_old_cap_against_the_dense_oracle(above, mode):
    out = above[mode]
    for b, (R, info) in enumerate(out):
        print(mode, b, R.shape[2], info["eig"], info["iters"], info["products"], info["residual"],
              aligned_diff(R, above[mode + "_ref"][b]), aligned_diff(R, above[mode + "_single"][b]))
    assert [info["eig"] for _, info in out] == ["lds", "streamed", "streamed", "streamed"]
    assert [R.shape[2] for R, _ in out] == [40, 279, 400, 748]
    for b, (R, info) in enumerate(out):
        assert info["converged"], (b, info)
        assert_rotations(R)
        assert aligned_diff(R, above[mode + "_ref"][b]) < 1e-8, (b, info)
        assert aligned_diff(R, above[mode + "_single"][b]) < 1e-8, (b, info)


def test_at_the_streamed_cap(lib):
    """n = desc_gcw_batch_streamed_max_n(): the launch declares the whole 160 KiB of LDS (the byte count of the LDS kernel at 278).
    Against the single calls, which take any size; behind a small problem, so that the launch covers a list of the batch."""
    from desc_amd import GCW, GCW_batch, Spectral, Spectral_batch
    mo, S = streamed.big("U1112")
    mo40, S40 = cases.mixed_models(lib.gcw_batch_max_n())[2], cases.mixed_S(lib.gcw_batch_max_n())[2]
    assert int(mo.Ind.max()) == lib.gcw_batch_streamed_max_n()
    for name, out, ref in (("gcw", GCW_batch([mo40, mo], [S40, S], return_info=True, eig="auto"), GCW(mo.Ind, None, mo.RijMat, S)),
                           ("spectral", Spectral_batch([mo40, mo], return_info=True, eig="auto"), Spectral(mo.Ind, mo.RijMat))):
        R, info = out[1]
        d = aligned_diff(R, ref)
        print(name, R.shape[2], info["eig"], info["iters"], info["products"], info["residual"], d)
        assert info["eig"] == "streamed" and out[0][1]["eig"] == "lds" and info["converged"], info
        assert_rotations(R)
        assert d < 1e-8, (name, d)


# ---- 3. composition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gcw", "spectral"])
def test_result_depends_on_neither_the_batch_nor_the_mode(above, mode):
    """As given, reversed, each problem alone (one launch instead of two, another LDS size), everything streamed: the same bits."""
    from desc_amd import GCW_batch, Spectral_batch
    mos, S = above["mos"], above["S"]

    def run(idx, **kw):
        if mode == "gcw":
            return GCW_batch([mos[b] for b in idx], [S[b] for b in idx], return_info=True, **kw)
        return Spectral_batch([mos[b] for b in idx], return_info=True, **kw)
    B = len(mos)
    rev = run(range(B - 1, -1, -1), eig="auto")
    all_streamed = run(range(B), eig="streamed")
    assert [info["eig"] for _, info in all_streamed] == ["streamed"] * B
    for b in range(B):
        assert same(above[mode][b], rev[B - 1 - b]), b
        assert same(above[mode][b], run([b], eig="auto")[0]), b
        assert same(above[mode][b], all_streamed[b]), b
    default = run([0])[0]
    assert default[1]["eig"] == "lds" and same(above[mode][0], default)


# ---- 4. handle reuse --------------------------------------------------------------------------------------------------------------
def test_handle_reuse(lib, above):
    mos = above["mos"][:3]
    probs = [arrays(lib, mo.Ind, mo.RijMat) for mo in mos]
    Sa = np.concatenate(above["S"][:3])
    Sb = np.concatenate([gs.noisy_truth(mo, 70 + k) for k, mo in enumerate(mos)])
    h = lib.GcwBatch(probs, eig="auto")
    first = h.run(s_vec=Sa)[0]
    second = h.run(s_vec=Sb)[0]
    again = h.run(s_vec=Sa)[0]
    h.destroy()
    for S, got in ((Sa, first), (Sb, second), (Sa, again)):
        fresh = handle_run(lib, probs, "auto", s_vec=S)
        assert all(same(a, b) for a, b in zip(got, fresh))
    assert all(same(a, b) for a, b in zip(first, above["gcw"][:3]))
    assert not any(same(a, b) for a, b in zip(first, second))


# ---- 5. the composites ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def composite(lib):
    from desc_amd import DESC_init_batch
    mos = streamed.composite_models()
    seeds = [3, 4]

    def par(seed=0):
        return dict(iters=30, Gradient=ConstantStepSize(0.01), seed=seed, verbose=False, build_where=lib.BUILD_HOST)
    return dict(mos=mos, seeds=seeds, par=par, init=DESC_init_batch(mos, par(), seeds=seeds, return_info=True, eig="auto"))


def test_desc_init_batch_auto(composite):
    from desc_amd import DESC_PGD_batch, DESC_init
    mos, seeds, par = composite["mos"], composite["seeds"], composite["par"]
    S_pgd = DESC_PGD_batch(mos, par(), seeds=seeds)
    assert [info["gcw"]["eig"] for _, _, info in composite["init"]] == ["lds", "streamed"]
    for b, (mo, (R, S_vec, info)) in enumerate(zip(mos, composite["init"])):
        assert np.array_equal(S_vec, S_pgd[b]), b
        assert info["pgd"]["iters_run"] == 30 and info["gcw"]["converged"], b
        assert_rotations(R)
        d = aligned_diff(R, gcw_oracle(mo.Ind, mo.RijMat, S_vec))
        R1, S1 = DESC_init(mo.Ind, mo.RijMat, par(seeds[b]))
        e, e1 = Rotation_Alignment(R, mo.R_orig)[2], Rotation_Alignment(R1, mo.R_orig)[2]
        print(b, d, e, e1, float(np.abs(S1 - S_vec).max()))
        assert d < 1e-8, (b, d)
        assert abs(e - e1) < 1e-6, (b, e, e1)


def test_desc_batch_auto(composite):
    from desc_amd import DESC_batch, DESC_refine_batch
    mos, seeds, par = composite["mos"], composite["seeds"], composite["par"]
    out = DESC_batch(mos, par(), seeds=seeds, return_info=True, eig="auto")
    assert [info["gcw"]["eig"] for *_, info in out] == ["lds", "streamed"]
    for b, ((R_est, R_init, S_vec, _), (R0, S0, _)) in enumerate(zip(out, composite["init"])):
        assert np.array_equal(R_init, R0) and np.array_equal(S_vec, S0), b
    refined = DESC_refine_batch(mos, [o[2] for o in out], [o[1] for o in out])
    for b, (R, o) in enumerate(zip(refined, out)):
        assert np.array_equal(R, o[0]), b
        assert_rotations(o[0])


def test_cemp_gcw_batch_auto():
    from desc_amd import CEMP_GCW, CEMP_GCW_batch, CEMP_batch
    mos = streamed.composite_models()
    probs = [(mo.Ind, mo.RijMat) for mo in mos]
    par = cemp_batch_cases.params()
    out = CEMP_GCW_batch(probs, par, return_info=True, eig="auto")
    S_cemp = CEMP_batch(probs, par)
    assert [info["gcw"]["eig"] for _, _, info in out] == ["lds", "streamed"]
    for b, ((R, S, info), prob) in enumerate(zip(out, probs)):
        assert np.array_equal(S, S_cemp[b]) and info["gcw"]["converged"], b
        assert_rotations(R)
        d = aligned_diff(R, CEMP_GCW(*prob, par))
        print(b, R.shape[2], info["gcw"]["iters"], d)
        assert d < 1e-8, (b, d)


def test_linprog_sij_batch_auto(lib):
    """max_iter = 256: the LP stops at its cap (one warning line), which is all the eigen-solve behind it needs."""
    from desc_amd import linprog_sij_batch
    mos = streamed.composite_models()
    probs = [(mo.Ind, mo.RijMat) for mo in mos]
    prm = dict(max_iter=256)
    out = linprog_sij_batch(probs, prm, return_info=True, eig="auto")
    S_lp = linprog_sij_batch(probs, prm, rotations=False)
    assert [info["spectral"]["eig"] for _, _, info in out] == ["lds", "streamed"]
    for b, (R_est, S_vec, info) in enumerate(out):
        assert np.array_equal(S_vec, S_lp[b]), b
        assert_rotations(R_est)
    gcw = handle_run(lib, [arrays(lib, mo.Ind, mo.RijMat) for mo in mos], "auto", weights=np.exp(-5.0 * np.concatenate(S_lp)),
                     normalize_rows=True)
    for b, ((R, _), (_, _, info)) in enumerate(zip(gcw, out)):
        assert np.array_equal(R, info["R_gcw"]), b

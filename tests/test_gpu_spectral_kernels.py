"""The kernels of the Spectral / GCW eigen-solve (desc_amd/csrc/spectral.hip) one at a time, through the desc_test_spectral_* hooks,
against the restatements of tests/spectral_kernels_oracle.py (qualified without a GPU by tests/test_spectral_host.py).  The hooks
launch through the functions spectral_impl launches with; a forced grid of 1 or 3 workgroups makes every stride loop turn on graphs
of a few hundred nodes.  A subspace iteration corrects itself, so none of this is visible end to end: a wrong shift term only filters
worse, a lost slot only costs products.

Bit-equal where the restatement follows the kernel's operation order (assembly, k_combine) and wherever the device is compared with
itself (two runs, forced grids against the product path's); elsewhere the bounds derived in the oracle module -- none is measured."""
import functools

import numpy as np
import pytest

from desc_amd import _lib as lib
from tests import spectral_cases as K
from tests import spectral_kernels_oracle as O

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def _dp(name):
    n, ii, jj, rij = K.graphs()[name]
    return lib.DeviceProblem(lib.ProblemArrays(n, ii, jj, np.ascontiguousarray(rij.reshape(-1))), 0)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------- assembly
@pytest.mark.parametrize("name", ["stars64", "stars256", "er60"])
@pytest.mark.parametrize("kind", ["unit", "wide", "dinv0"])
def test_assembly_is_the_restatement_bit_for_bit(name, kind):
    n, ii, jj, rij = K.graphs()[name]
    w = K.edge_weights(len(ii), "wide") if kind != "unit" else None
    dinv = K.dinv_with_zeros(n) if kind == "dinv0" else None
    want = O.assemble(n, ii, jj, rij, w, dinv)
    got = {g: lib.hook_spectral_assemble(_dp(name), w, dinv, grid=g) for g in K.GRIDS}
    for g in K.GRIDS:
        assert _same_bits(got[g], want), (name, kind, g)
    A = O.dense_from_blocks(n, ii, jj, got[0])
    assert np.array_equal(A, A.T)                                      # block (v, u) is exactly the transpose of block (u, v)
    if kind == "dinv0":
        dead = np.flatnonzero(dinv == 0)
        assert not A.reshape(n, 3, n, 3)[dead].any() and not A.reshape(n, 3, n, 3)[:, :, dead].any()


# ---------------------------------------------------------------------------------------------------------------- spmm
def _spmm_inputs(name, pname):
    n, ii, jj, rij = K.graphs()[name]
    alpha, s1, s2, zk, z_is_y = K.spmm_params()[pname]
    blocks = O.assemble(n, ii, jj, rij, K.edge_weights(len(ii), "wide") if name == "er60" else None)
    x = K.operand(n, 1)
    z = x if zk == "x" else K.operand(n, 2) if zk == "other" else np.full_like(x, np.nan)
    return n, ii, jj, blocks, x, z, alpha, s1, s2, z_is_y


@pytest.mark.parametrize("name", ["stars64", "stars256", "er60"])
@pytest.mark.parametrize("pname", list(K.spmm_params()))
def test_spmm_forms_and_grids(name, pname):
    n, ii, jj, blocks, x, z, alpha, s1, s2, z_is_y = _spmm_inputs(name, pname)
    want, bound = O.spmm(n, ii, jj, blocks, x, z, alpha, s1, s2)
    dp = _dp(name)
    run = lambda form, grid: lib.hook_spectral_spmm(dp, blocks, x, z, alpha, s1, s2, z_is_y=z_is_y, form=form, grid=grid)
    prod = run(0, 0)
    assert _same_bits(prod, run(0, 0))                                 # two runs
    assert _same_bits(prod, run(64, 0))                                # the product path's rule picks the wave-per-row kernel on these graphs
    for form in (64, 256, 2):
        y0 = run(form, 0)
        err = np.abs(y0 - want)
        assert np.isfinite(y0).all() and (err <= bound).all(), (name, pname, form, float((err / np.maximum(bound, 1e-300)).max()))
        for g in (1, 3):
            assert _same_bits(run(form, g), y0), (name, pname, form, g)
        if name == "stars64":                                          # the isolated node: no slot, exactly s1 x + s2 z
            v = K.star_forest(K.LEAVES_64)[4][0]
            rows = slice(3 * v, 3 * v + 3)
            exact = alpha * 0.0 + s1 * x[rows] + (s2 * z[rows] if s2 != 0.0 else 0.0)
            assert _same_bits(y0[rows], exact), (pname, form)


# ---------------------------------------------------------------------------------------------------------------- weights, row sums
def test_gcw_weights_at_the_special_values():
    S = np.array(K.S_VALUES + tuple(np.random.default_rng(3).uniform(2e-3, 1.0, size=300)))
    got = lib.hook_spectral_weights(S)
    want = O.gcw_weights(S)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan[6] and nan[7] and nan.sum() == 2
    assert got[5] == 0.0                                               # S = +inf
    # 16 ulp for pow (the OpenCL full-profile bound the device pow is written to) + the add + the divide
    assert (np.abs(got[~nan] - want[~nan]) <= 18 * EPS * np.abs(want[~nan])).all(), np.abs(got[~nan] / want[~nan] - 1).max() / EPS


@pytest.mark.parametrize("name", ["tiny1", "tiny2", "tiny3", "tiny5", "tiny64", "tiny67", "stars64", "stars256"])
@pytest.mark.parametrize("kind", ["unit", "wide"])
def test_row_sums(name, kind):
    if name.startswith("tiny"):
        n, ii, jj, rij = K.tiny_graph(int(name[4:]))
        dp = lib.DeviceProblem(lib.ProblemArrays(n, ii, jj, np.ascontiguousarray(rij.reshape(-1))), 0)
    else:
        n, ii, jj, rij = K.graphs()[name]
        dp = _dp(name)
    w = K.edge_weights(len(ii), kind)
    want, bound = O.row_wsum(n, ii, jj, w)
    got = {g: lib.hook_spectral_row_wsum(dp, w, grid=g) for g in K.GRIDS}      # grid 1: 16 rows per turn, a row block is revisited
    assert (np.abs(got[0] - want) <= bound).all(), float((np.abs(got[0] - want) / np.maximum(bound, 1e-300)).max())
    if kind == "unit":
        assert np.array_equal(got[0], want)                            # small integers: exact in any order
    for g in (1, 3):
        assert _same_bits(got[g], got[0]), (name, kind, g)
    if name.startswith("tiny"):
        dp.free()


# ---------------------------------------------------------------------------------------------------------------- gram, residual, combine
@functools.lru_cache(maxsize=None)
def _blocks(rows):
    rng = np.random.default_rng(rows)
    X, Y = rng.uniform(-1, 1, size=(rows, 6)), rng.uniform(-1, 1, size=(rows, 6))
    return X, Y, rng.standard_normal((6, 3)), rng.standard_normal(3), rng.standard_normal((6, 6))


@pytest.mark.parametrize("rows", K.ROW_COUNTS)
def test_gram(rows):
    X, Y, _, _, _ = _blocks(rows)
    G1, G2, b1, b2 = O.gram(X, Y)
    got = {g: lib.hook_spectral_gram(X, Y, grid=g) for g in K.GRIDS}
    for g in K.GRIDS:
        assert (np.abs(got[g][0] - G1) <= b1).all() and (np.abs(got[g][1] - G2) <= b2).all(), (rows, g)
    assert _same_bits(got[0][0], lib.hook_spectral_gram(X, Y)[0])
    assert np.array_equal(got[0][1], got[0][1].T)                      # y_a y_b and y_b y_a are the same products in the same order


@pytest.mark.parametrize("rows", K.ROW_COUNTS)
def test_residual(rows):
    X, Y, Z3, theta, _ = _blocks(rows)
    want, bound = O.residual(X, Y, Z3, theta)
    for g in K.GRIDS:
        got = np.sqrt(lib.hook_spectral_residual(X, Y, Z3, theta, grid=g))
        assert (np.abs(got - want) <= bound).all(), (rows, g, np.abs(got - want) / bound)
    assert _same_bits(lib.hook_spectral_residual(X, Y, Z3, theta), lib.hook_spectral_residual(X, Y, Z3, theta))


@pytest.mark.parametrize("rows", [257, 65537])
def test_residual_keeps_two_digits_next_to_an_eigenpair(rows):
    """Y = X diag(lambda) + a perturbation of 1e-12 relative: the explicit residual sees it to two digits (the bound says so before
    anything is measured); z'G2 z - theta^2 would not."""
    X, Y, Z3, theta = K.residual_near_eigenpair(rows)
    want, bound = O.residual(X, Y, Z3, theta)
    assert (bound <= 1e-2 * want).all()
    got = np.sqrt(lib.hook_spectral_residual(X, Y, Z3, theta))
    assert (np.abs(got - want) <= bound).all() and (np.abs(got - want) <= 1e-2 * want).all()


@pytest.mark.parametrize("rows", K.ROW_COUNTS)
def test_combine_is_the_restatement_bit_for_bit(rows):
    _, Y, _, _, Cm = _blocks(rows)
    want = O.combine(Y, Cm)
    for g in K.GRIDS:
        assert _same_bits(lib.hook_spectral_combine(Y, Cm, grid=g), want), (rows, g)

"""linprog_sij (Algorithms/linprog_sij.m) and DESC_init without a GPU: the new ABI, self-checks of the restatement (tests/lp_oracle.py)
against HiGHS through duality -- the LP optimum is not unique, so no vector is compared element by element -- and argument checks."""
import ctypes as C

import numpy as np
import pytest

from desc_amd.models import Uniform_Topology
from tests import lp_oracle as O


def test_lp_abi_symbols_structs_and_defaults(lib):
    L = lib.load()
    for name in ("desc_lp_params_default", "desc_lp_sij_run", "desc_lp_sij_run_dev"):
        assert hasattr(L, name) and name in lib.EXPORTS
    assert C.sizeof(lib.LpParams) == 48 and C.sizeof(lib.LpInfo) == 104          # as include/desc_amd.h states
    p = lib.default_lp_params()
    assert (p.nsample, p.seed, p.tol, p.max_iter, p.check_every, p.restart, p.verbose) == (0, 0, 1e-4, 200000, 64, 1, 0)
    assert not p.pos_out


@pytest.fixture(scope="module", params=[(30, 0.2), (30, 0.3), (60, 0.2), (60, 0.3)], ids=["n30-q0.2", "n30-q0.3", "n60-q0.2", "n60-q0.3"])
def lp(request):
    n, q = request.param
    mo = Uniform_Topology(n, 0.5, q, 0.05, "uniform", seed=3)
    K, b, pos, k, ns = O.build_lp(mo.Ind, mo.RijMat, 3)
    return mo, K, b, pos, k, ns, O.solve_highs(K, b)


def test_oracle_lp_shape(lp):
    mo, K, b, pos, k, ns, _ = lp
    mp = pos.size
    assert ns == 30 and K.shape == (2 * ns * mp, mp) and k.shape == (mp, ns) and b.shape == (2 * ns * mp,)
    assert np.array_equal(np.asarray(abs(K).sum(axis=1)).reshape(-1), np.full(K.shape[0], 3.0))
    assert np.all(b[0::2] == -b[1::2]) and np.all(b[0::2] >= 0)
    i, j = mo.Ind[pos, 0], mo.Ind[pos, 1]
    assert np.all(k != i[:, None]) and np.all(k != j[:, None]) and k.min() >= 1 and k.max() <= mo.Ind.max()


def test_oracle_certificates_close_on_the_highs_optimum(lp):
    _, K, b, _, _, _, (f, x, y) = lp
    assert np.all(y >= 0) and np.all(x >= 0) and np.all(x <= 1)
    viol, P, D = O.certificates(K, b, x, y)
    print("viol %.3e  P %.12g  D %.12g  f* %.12g" % (viol, P, D, f))
    assert viol <= 1e-9
    assert abs(P - D) <= 1e-7 * (1 + f)


def test_oracle_plain_pdhg_stays_inside_the_duality_bounds(lp):
    """Every y >= 0 is dual feasible (D <= f*), and weak duality against HiGHS's dual bounds P from below:
    c'x + y*'(Kx - b) >= min over the box = f*."""
    _, K, b, _, _, _, (f, xs, ys) = lp
    tau, sigma = O.step_sizes(K)
    assert np.all(sigma == 1.0 / 3.0)
    for N in (1, 50, 2000):
        x, y = O.pdhg_plain(K, b, tau, sigma, N)
        assert np.all(y >= 0) and np.all(x >= 0) and np.all(x <= 1)
        viol, P, D = O.certificates(K, b, x, y)
        print("N %d: viol %.3e  P %.9g  D %.9g  f* %.9g" % (N, viol, P, D, f))
        assert D <= f + 1e-9 * (1 + f)
        assert P >= f - ys @ np.maximum(K @ x - b, 0.0) - 1e-9 * (1 + f)
    assert abs(P - f) < 0.05 * f and viol < 0.05          # 2000 steps: on its way (the bounds above hold at any step)


def test_oracle_edges_without_a_cycle_are_no_variables():
    Ind = np.array([[1, 2], [1, 3], [2, 3], [3, 4], [4, 5]])            # a triangle with a tail
    R = np.repeat(np.eye(3)[:, :, None], 5, axis=2)
    K, b, pos, k, ns = O.build_lp(Ind, R, 0, nsample=4)
    assert list(pos) == [0, 1, 2] and K.shape == (24, 3) and np.all(b == 0)
    assert np.array_equal(k, np.array([[3] * 4, [2] * 4, [1] * 4]))
    assert O.rule_nsample([1, 1, 1]) == 30 and O.rule_nsample([200, 210, 220]) == 53 and O.rule_nsample([]) == 30


def test_linprog_sij_and_desc_init_check_their_arguments():
    from desc_amd import DESC_init, linprog_sij
    from desc_amd import ConstantStepSize
    params = dict(iters=5, Gradient=ConstantStepSize(0.01), verbose=False)
    R0 = np.zeros((3, 3, 0))
    for call in (lambda I, R: linprog_sij(I, R), lambda I, R: DESC_init(I, R, params)):
        with pytest.raises(ValueError, match="empty edge list"):
            call(np.zeros((0, 2), dtype=np.int64), R0)
        with pytest.raises(ValueError, match="m x 2"):
            call(np.array([1, 2, 3]), R0)
        with pytest.raises(ValueError, match="3 x 3 x m"):
            call(np.array([[1, 2], [1, 3]]), np.zeros((3, 3, 5)))
        with pytest.raises(ValueError):
            call(np.array([[2, 1]]), np.zeros((3, 3, 1)))               # Ind(:,1) < Ind(:,2)

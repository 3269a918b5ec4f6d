"""GPU tests of the batched rotation alignment (csrc/align_batch.hip, Rotation_Alignment_batch): the projection hook alone, every case
of tests/align_batch_cases.py against Rotation_Alignment per problem, the inverse check of the errors, the exact kind's bound, the
summation order of mean_error and the median rule bit for bit, independence of the batch, and the call's usage.

Tolerances.  tests/align_batch_oracle.py restates the call with the device's Jacobi SVD and summation orders.  Run on the CPU over all
the cases, it differs from Rotation_Alignment (LAPACK's SVD, NumPy's sums) by at most
    R_align 1.84e-14, R_out 1.90e-14, err (nodes above 1e-3 degrees) 7.91e-12 degrees, mean 3.45e-12, median 3.41e-12 degrees
(align_batch_cases.MEASURED holds these rounded up; tests/test_align_batch_host.py repeats the measurement).  The device may differ from
Rotation_Alignment by 16 times as much (align_batch_cases.TOL) -- the margin is for the device's acos and sqrt against libm's:
    R_align 3.04e-13, R_out 3.04e-13, err 1.28e-10 degrees, mean 5.6e-11, median 5.6e-11 degrees.
On an MI355X the device's differences were the restatement's own, digit for digit (1.83e-14, 1.90e-14, 7.90e-12, 3.44e-12, 3.41e-12).
mean and median are compared this way on the problems whose reference median exceeds 1e-3 degrees; the others are exact alignments
(the exact and constant kinds), where acos is ill-conditioned and both answers must lie in [0, 6.8e-6 degrees] instead."""
import numpy as np
import pytest

from tests import align_batch_cases as cases
from tests import align_batch_oracle as O

pytestmark = pytest.mark.gpu

_ran = {}


def ran(which):
    """Rotation_Alignment_batch(..., return_info=True) of 'single' | 'mixed' | 'many', run once and shared (treat as read-only)."""
    if which not in _ran:
        from desc_amd import Rotation_Alignment_batch
        probs = dict(single=list(cases.SINGLE.values()), mixed=cases.MIXED, many=cases.MANY)[which]
        _ran[which] = Rotation_Alignment_batch([E for E, _ in probs], [G for _, G in probs], return_info=True)
    return _ran[which]


def problems(which):
    return dict(single=list(cases.SINGLE.values()), mixed=cases.MIXED, many=cases.MANY)[which]


def _same(a, b, rotations=True):
    """Two results of one problem are the same bits (R_out only where both hold one)."""
    ok = np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3] and np.array_equal(a[4]["err"], b[4]["err"])
    return ok and (not rotations or np.array_equal(a[0], b[0]))


def test_projection_hook(lib):
    assert lib.GUARD
    rng = np.random.default_rng(77)
    blocks = rng.standard_normal((1100, 3, 3))
    s = np.linalg.svd(blocks, compute_uv=False)
    gap = (s[:, 1] + np.sign(np.linalg.det(blocks)) * s[:, 2]) / s[:, 0]
    blocks = blocks[gap >= cases.GAP_MIN][:1000]
    assert blocks.shape[0] == 1000 and (np.linalg.det(blocks) < 0).sum() > 300
    grams = np.array([cases.gram(E, G)[0] for _, E, G in cases.every_problem()])
    A = np.concatenate([blocks, grams])
    A9 = np.transpose(A, (0, 2, 1)).reshape(-1, 9)                                           # column-major blocks
    got = lib.hook_align_project(A9)
    U, _, Vt = np.linalg.svd(A)
    U[:, :, 2] *= np.linalg.det(U @ Vt)[:, None]
    want = np.transpose(U @ Vt, (0, 2, 1)).reshape(-1, 9)
    scale = 1.0 / np.concatenate([gap[gap >= cases.GAP_MIN][:1000], [cases.gram(E, G)[1] for _, E, G in cases.every_problem()]])
    d = np.abs(got - want).max(axis=1)
    print(f"projection hook: max |device - LAPACK| = {d.max():.3e}, times the gap {np.max(d / scale):.3e}")
    # a perturbation dA of A moves the projection by at most 2 |dA| / (s2 +- s3), i.e. (2 / gap) |dA| / s1; each of the two SVDs is
    # backward stable to a few tens of ulps of s1 (3x3, at most ten Jacobi sweeps): 2 * 128 ulps = 2^-45 in all
    assert np.max(d / scale) <= 2.0 ** -45
    R = got.reshape(-1, 3, 3)
    assert np.abs(R @ np.transpose(R, (0, 2, 1)) - np.eye(3)).max() <= 1e-13 and np.abs(np.linalg.det(R) - 1).max() <= 1e-13
    # the restatement holds the same text: the same bits where the device's sqrt and division round as libm's, and 16 ulps times the
    # projection's condition 1 / gap where they are an ulp apart
    assert np.max(np.abs(got - O.project_blocks(A9)).max(axis=1) / scale) <= 16 * 2.0 ** -52


@pytest.mark.parametrize("which", ["single", "mixed", "many"])
def test_against_rotation_alignment(lib, which):
    assert lib.GUARD                                             # every buffer of the run was fenced and verified
    worst = dict.fromkeys(cases.TOL, 0.0)
    for b, (got, ref, (E, G)) in enumerate(zip(ran(which), cases.reference(which), problems(which))):
        R_out, R_align, mean, median, info = got
        r_out, r_align, r_mean, r_median, r_err = ref
        n = E.shape[2]
        assert R_out.shape == (3, 3, n) and R_out.flags.f_contiguous and R_align.shape == (3, 3) and info["err"].shape == (n,)
        assert isinstance(mean, float) and isinstance(median, float)
        big = r_err > 1e-3
        d = dict(R_align=np.abs(R_align - r_align).max(), R_out=np.abs(R_out - r_out).max(), err=np.abs(info["err"] - r_err)[big].max(initial=0.0))
        if r_median > 1e-3:
            d.update(mean=abs(mean - r_mean), median=abs(median - r_median))
        else:
            assert 0 <= mean <= cases.EXACT_MAX and 0 <= median <= cases.EXACT_MAX, (which, b)
        for k, v in d.items():
            worst[k] = max(worst[k], float(v))
    print(f"{which}: max |device - Rotation_Alignment| = {worst}")
    for k, v in worst.items():
        assert v <= cases.TOL[k], (which, k, v)


@pytest.mark.parametrize("which", ["single", "mixed", "many"])
def test_inverse_check(which):
    """cos(err) against the trace formed in NumPy from the returned R_out: free of acos's conditioning near 0."""
    eye = np.eye(3)
    for b, ((R_out, R_align, _, _, info), (E, G)) in enumerate(zip(ran(which), problems(which))):
        tr = np.einsum("abk,abk->k", G, R_out)
        assert np.abs(np.cos(info["err"] * np.pi / 180) - (tr - 1) / 2).max() <= 1e-13, (which, b)
        assert (info["err"] >= 0).all() and (info["err"] <= 180 + 1e-5).all()
        assert np.abs(np.einsum("abk,ack->kbc", R_out, R_out) - eye).max() <= 1e-13, (which, b)
        assert abs(np.linalg.det(R_align) - 1) <= 1e-13 and np.abs(R_align.T @ R_align - eye).max() <= 1e-13, (which, b)
        assert np.abs(R_out - np.einsum("abk,bc->ack", E, R_align)).max() <= 1e-15, (which, b)


def test_exact_kind():
    seen = 0
    for name, got in zip(cases.SINGLE, ran("single")):
        if name.startswith(("exact", "constant")):
            seen += 1
            assert got[4]["err"].max() <= cases.EXACT_MAX and got[2] <= cases.EXACT_MAX and got[3] <= cases.EXACT_MAX, name
    assert seen == 2 * len(cases.SIZES)


@pytest.mark.parametrize("which", ["single", "mixed", "many"])
def test_mean_and_median_bit_for_bit(which):
    for b, (_, _, mean, median, info) in enumerate(ran(which)):
        assert mean == O.mean_error(info["err"]), (which, b)
        assert median == O.median_error(info["err"]), (which, b)


def test_constant_and_two_class():
    by_name = dict(zip(cases.SINGLE, ran("single")))
    for n in cases.SIZES:
        _, _, mean, median, info = by_name[f"constant-{n}"]
        assert (info["err"] == median).all(), n                              # all errors the same bits: the flat and ties path
    for n in (256, 257):
        _, _, _, median, info = by_name[f"two-class-{n}"]
        h = (n + 1) // 2
        a, b = info["err"][:h], info["err"][h:]
        assert np.unique(a).size == 1 and np.unique(b).size == 1 and a[0] > 10 and b[0] > 10
        lo, hi = min(a[0], b[0]), max(a[0], b[0])
        if n == 256:
            assert median == lo + (hi - lo) / 2.0                            # the median straddles the two runs
        else:
            assert median == a[0]                                            # ... or sits inside the longer one (129 of 257)


def test_independence_of_the_batch():
    from desc_amd import Rotation_Alignment_batch as RAB
    mixed = ran("mixed")
    order = [3, 0, 4, 2, 1]
    moved = RAB([cases.MIXED[b][0] for b in order], [cases.MIXED[b][1] for b in order], return_info=True)
    for pos, b in enumerate(order):
        E, G = cases.MIXED[b]
        alone = RAB([E], [G], return_info=True)[0]
        assert _same(alone, mixed[b]), b                                                    # alone
        assert _same(alone, moved[pos]), b                                                  # at another position of the batch
    for b in (0, 137, 299):                                                                 # inside the B = 300 batch
        E, G = cases.MANY[b]
        assert _same(RAB([E], [G], return_info=True)[0], ran("many")[b]), b
    # without rotations: the same bits, and no R_out
    bare = RAB([E for E, _ in cases.MIXED], [G for _, G in cases.MIXED], rotations=False, return_info=True)
    for b in range(len(cases.MIXED)):
        assert bare[b][0] is None and _same(bare[b], mixed[b], rotations=False), b
    plain = RAB([E for E, _ in cases.MIXED], [G for _, G in cases.MIXED])
    assert all(len(t) == 4 and np.array_equal(t[0], m[0]) and t[2] == m[2] for t, m in zip(plain, mixed))


def test_two_runs_on_one_handle(lib):
    """A second run of the same estimates gives the same bits; a run with other estimates scores against the same ground truth."""
    n = [E.shape[2] for E, _ in cases.MIXED]
    est = np.concatenate([E.reshape(-1, order="F") for E, _ in cases.MIXED])
    gt = np.concatenate([G.reshape(-1, order="F") for _, G in cases.MIXED])
    h = lib.AlignBatch(n, gt)
    try:
        assert h.count == 5 and h.node_off.tolist() == np.concatenate([[0], np.cumsum(n)]).tolist()
        first, tm = h.run(est)
        other, _ = h.run(gt, rotations=False)                                              # the truth itself: exact alignments
        again, _ = h.run(est)
    finally:
        h.destroy()
    assert set(tm) == {"ms_upload", "ms_align", "ms_copy", "ms_total"} and all(v > 0 for v in tm.values())
    assert tm["ms_total"] >= tm["ms_upload"] + tm["ms_align"] + tm["ms_copy"]
    for k in first:
        assert np.array_equal(first[k], again[k]), k
    assert other["R_out"] is None and other["err"].max() <= cases.EXACT_MAX
    for b, got in enumerate(ran("mixed")):
        n0, n1 = int(h.node_off[b]), int(h.node_off[b + 1])
        assert np.array_equal(first["err"][n0:n1], got[4]["err"]) and first["mean_error"][b] == got[2]
        assert np.array_equal(first["R_out"][9 * n0:9 * n1].reshape((3, 3, n1 - n0), order="F"), got[0])


def test_models_and_memory_orders():
    """Models from Uniform_Topology_batch are accepted as R_gt_list; arrays may be in any memory order."""
    from desc_amd import Rotation_Alignment, Rotation_Alignment_batch, Uniform_Topology_batch
    mos = Uniform_Topology_batch([30, 65], 0.5, 0.2, 0.1, seeds=[5, 6])
    rng = np.random.default_rng(9)
    ests = [np.ascontiguousarray(np.einsum("abk,bc->ack", mo.R_orig, cases.haar(rng, 1)[0])) for mo in mos]      # C order
    assert not ests[0].flags.f_contiguous
    out = Rotation_Alignment_batch(ests, mos, rotations=False)
    arr = Rotation_Alignment_batch([np.asfortranarray(e) for e in ests], [mo.R_orig for mo in mos])
    for (R_out, R_align, mean, median), a, e, mo in zip(out, arr, ests, mos):
        assert R_out is None and np.array_equal(R_align, a[1]) and mean == a[2] and median == a[3]
        assert mean <= cases.EXACT_MAX and np.abs(a[0] - mo.R_orig).max() <= 1e-14
        assert np.abs(R_align - Rotation_Alignment(e, mo.R_orig)[1]).max() <= cases.TOL["R_align"]

"""Every instance of the PGD sweep (DESC_PGD.m:185-230) against the CPU oracle, on both sides of each size edge of its dispatch.

Which instance runs depends on the longest segment (max_cnt: cycles per edge) crossing 16, 32, 64, 128 and 256, on the step kind (STEP 0:
constant, piecewise and hybrid-plain steps; STEP 2: Adam), on the layout (gather / small / node / band) and on whether the handle is one
rank or a shard.  max_cnt is pinned by n_sample_min = T: n_sample = max(ceil(median(codeg) / 4), n_sample_min) (DESC_PGD.m:43), so on a
dense graph whose median codegree is at most 4 T and whose largest is at least T the longest segment has exactly T cycles.

One table: the graph, T, the layout forced, the step kind, the world (1, or 2 / 3 / 8 ranks emulated on one card) and the exact
instance the case must launch.  test_table_covers_every_instance (CPU) parses the instance set out of the sweep units (sweep_gather.hip,
sweep_node.hip, sweep_band.hip) and checks that T is what the oracle's structure gives; the GPU cases then only have to confirm the
dispatch and the numbers."""
import functools
import os
import re

import numpy as np
import pytest

from tests.helpers import (assert_structure_equal, c_params, emulate_sharded, make_problem, run_unsharded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
# T (and T + 1) -> Uniform_Topology(n, p, 0.2, 0.1, "uniform", seed=1): median codegree <= 4 T, largest >= T + 1
GRAPHS = {16: (80, 0.7), 32: (120, 0.7), 64: (200, 0.8), 128: (200, 0.9), 256: (330, 0.97)}
STEPS = dict(const=dict(step_kind=0, lr=0.01),
             piecewise=dict(step_kind=1, lr=0.05, decay_interval=7, t0=3),
             hybrid_plain=dict(step_kind=2, lr=0.0005, decay_interval=10, hybrid_strategy=1, t0=4),      # STEP 0 kernels, step from the host
             adam=dict(step_kind=2, lr=0.001, beta1=0.9, beta2=0.999, decay_interval=10))
# DESC_DEBUG_VARIANT per layout: auto = the library's own choice (k_sweep_small below 2 M cycles and 65 cycles), band-j = band sweep with
# j-block-major units (17..32 cycles: k_sweep_band<16,2> instead of <8,4>)
LAYOUTS = {"auto": {}, "gather": dict(DESC_DEBUG_VARIANT="1"), "node": dict(DESC_DEBUG_VARIANT="2"), "band": dict(DESC_DEBUG_VARIANT="3"),
           "band-j": dict(DESC_DEBUG_VARIANT="3", DESC_DEBUG_JMAJOR="1")}

# (layout, T, step, world, the sweep instance it must launch)
CASES = [
    # gather layout: G = 16 / 32 / 64 cycles per lane group, the multi-pass wave-per-edge kernel above 64
    ("gather", 16, "const", 1, "k_sweep<16,0>"),
    ("gather", 16, "adam", 1, "k_sweep<16,2>"),
    ("gather", 17, "const", 1, "k_sweep<32,0>"),
    ("gather", 32, "adam", 1, "k_sweep<32,2>"),
    ("gather", 33, "adam", 1, "k_sweep<64,2>"),
    ("gather", 64, "const", 1, "k_sweep<64,0>"),
    ("gather", 65, "const", 1, "k_sweep_big<0>"),
    ("gather", 65, "adam", 1, "k_sweep_big<2>"),
    # the library's own choice: the small-graph sweep up to 64 cycles, k_sweep_node above; band sweep from 2 M cycles up to 256, gather above
    ("auto", 16, "const", 1, "k_sweep_small<16,0>"),
    ("auto", 16, "adam", 1, "k_sweep_small<16,2>"),
    ("auto", 17, "adam", 1, "k_sweep_small<32,2>"),
    ("auto", 17, "piecewise", 1, "k_sweep_small<32,0>"),
    ("auto", 32, "const", 1, "k_sweep_small<32,0>"),
    ("auto", 33, "const", 1, "k_sweep_small<64,0>"),
    ("auto", 64, "adam", 1, "k_sweep_small<64,2>"),
    ("auto", 65, "const", 1, "k_sweep_node<32,4,0>"),
    ("auto", 256, "const", 1, "k_sweep_band<64,4,0,512,one-rank>"),
    ("auto", 257, "const", 1, "k_sweep_big<0>"),
    # node layout, one rank: lanes per segment x cycles per lane
    ("node", 16, "const", 1, "k_sweep_node<16,1,0>"),
    ("node", 16, "adam", 1, "k_sweep_node<16,1,2>"),
    ("node", 17, "const", 1, "k_sweep_node<16,2,0>"),
    ("node", 17, "hybrid_plain", 1, "k_sweep_node<16,2,0>"),
    ("node", 32, "adam", 1, "k_sweep_node<16,2,2>"),
    ("node", 33, "const", 1, "k_sweep_node<32,2,0>"),
    ("node", 33, "adam", 1, "k_sweep_node<32,2,2>"),
    ("node", 64, "const", 1, "k_sweep_node<32,2,0>"),
    ("node", 65, "const", 1, "k_sweep_node<32,4,0>"),
    ("node", 65, "adam", 1, "k_sweep_node<32,4,2>"),
    ("node", 128, "const", 1, "k_sweep_node<32,4,0>"),
    ("node", 129, "const", 1, "k_sweep_node<64,4,0>"),
    ("node", 129, "adam", 1, "k_sweep_node<64,4,2>"),
    # node layout, sharded
    ("node", 16, "const", 2, "k_sweep_node<16,1,0> sharded"),
    ("node", 16, "adam", 3, "k_sweep_node<16,1,2> sharded"),
    ("node", 17, "const", 3, "k_sweep_node<16,2,0> sharded"),
    ("node", 32, "adam", 2, "k_sweep_node<16,2,2> sharded"),
    ("node", 33, "const", 2, "k_sweep_node<32,2,0> sharded"),
    ("node", 33, "adam", 3, "k_sweep_node<32,2,2> sharded"),
    ("node", 64, "const", 8, "k_sweep_node<32,2,0> sharded"),
    ("node", 65, "const", 3, "k_sweep_node<32,4,0> sharded"),
    ("node", 65, "adam", 2, "k_sweep_node<32,4,2> sharded"),
    ("node", 129, "const", 2, "k_sweep_node<64,4,0> sharded"),
    ("node", 129, "adam", 3, "k_sweep_node<64,4,2> sharded"),
    # band sweep, one rank
    ("band", 16, "const", 1, "k_sweep_band<16,1,0,1024,one-rank>"),
    ("band", 17, "const", 1, "k_sweep_band<8,4,0,512,one-rank>"),
    ("band-j", 17, "const", 1, "k_sweep_band<16,2,0,512,one-rank>"),
    ("band", 32, "const", 1, "k_sweep_band<8,4,0,512,one-rank>"),
    ("band-j", 32, "const", 1, "k_sweep_band<16,2,0,512,one-rank>"),
    ("band", 33, "const", 1, "k_sweep_band<16,4,0,512,one-rank>"),
    ("band", 64, "const", 1, "k_sweep_band<16,4,0,512,one-rank>"),
    ("band", 65, "const", 1, "k_sweep_band<32,4,0,512,one-rank>"),
    ("band", 128, "const", 1, "k_sweep_band<32,4,0,512,one-rank>"),
    ("band", 129, "const", 1, "k_sweep_band<64,4,0,512,one-rank>"),
    ("band", 16, "adam", 1, "k_sweep_band<16,1,2,512,one-rank>"),
    ("band", 17, "adam", 1, "k_sweep_band<16,2,2,512,one-rank>"),
    ("band", 32, "adam", 1, "k_sweep_band<16,2,2,512,one-rank>"),
    ("band", 33, "adam", 1, "k_sweep_band<32,2,2,512,one-rank>"),
    ("band", 64, "adam", 1, "k_sweep_band<32,2,2,512,one-rank>"),
    ("band", 65, "adam", 1, "k_sweep_node<32,4,2>"),                  # Adam above 64 cycles: the band handle sweeps with k_sweep_node
    # band sweep, sharded (XT: exchange positions per segment, S into the all-gather slice)
    ("band", 16, "const", 2, "k_sweep_band<16,1,0,1024,XT>"),
    ("band", 17, "const", 3, "k_sweep_band<8,4,0,512,XT>"),
    ("band-j", 17, "const", 2, "k_sweep_band<16,2,0,512,XT>"),
    ("band", 32, "const", 2, "k_sweep_band<8,4,0,512,XT>"),
    ("band-j", 32, "const", 3, "k_sweep_band<16,2,0,512,XT>"),
    ("band", 33, "const", 8, "k_sweep_band<16,4,0,512,XT>"),
    ("band", 33, "piecewise", 2, "k_sweep_band<16,4,0,512,XT>"),
    ("band", 64, "const", 3, "k_sweep_band<16,4,0,512,XT>"),
    ("band", 65, "const", 2, "k_sweep_band<32,4,0,512,XT>"),
    ("band", 128, "const", 3, "k_sweep_band<32,4,0,512,XT>"),
    ("band", 129, "const", 2, "k_sweep_band<64,4,0,512,XT>"),
    ("band", 16, "adam", 3, "k_sweep_band<16,1,2,512,XT>"),
    ("band", 17, "adam", 2, "k_sweep_band<16,2,2,512,XT>"),
    ("band", 32, "adam", 3, "k_sweep_band<16,2,2,512,XT>"),
    ("band", 33, "adam", 2, "k_sweep_band<32,2,2,512,XT>"),
    ("band", 64, "adam", 8, "k_sweep_band<32,2,2,512,XT>"),
    ("band", 65, "adam", 3, "k_sweep_node<32,4,2> sharded"),
]


def _case_id(c):
    layout, T, step, world, _ = c
    return f"{layout}-T{T}-{step}-w{world}"


def _base(T):
    return T if T in GRAPHS else T - 1


def _iters(T):
    return 20 if T <= 65 else 10


@functools.lru_cache(maxsize=None)
def _graph(base):
    n, p = GRAPHS[base]
    return make_problem("uniform", n=n, p=p, q=0.2, sigma=0.1, seed=1)


@functools.lru_cache(maxsize=None)
def _reference(O, T, step):
    """Oracle structure (structure seed 0, n_sample_min = T), S0 and run, shared by every case of the same graph, T and step."""
    mo, nn, ii, jj, rij = _graph(_base(T))
    st = O.build_structure(nn, ii, jj, seed=0, n_sample_min=T)
    S0 = O.cycle_d(ii, jj, rij.reshape(-1, 9), st)
    return st, S0, O.pgd_run(st, S0, _iters(T), **STEPS[step])


# ------------------------------------------------------------------------------------------------------------------ CPU guard
def _instances():
    """Every sweep instance the dispatch can launch, named as desc_debug_last_sweep names them: the entries <family>_inst<...>() of the
    instance tables (sweep_gather.hip, sweep_node.hip, sweep_band.hip), each standing for its two step kinds (band sweep: for one rank
    and XT)."""
    csrc = os.path.join(ROOT, "desc_amd", "csrc")
    units = sorted(nm for nm in os.listdir(csrc) if nm.endswith((".hip", ".cpp", ".h")))          # every unit of the library
    assert {"pgd.hip", "pgd_layout.hip", "pgd_shard.hip", "pgd_ext.hip", "pgd_handle.h", "sweep_gather.hip", "sweep_node.hip", "sweep_band.hip"} <= set(units)
    code = []
    for nm in units:
        with open(os.path.join(csrc, nm)) as f:
            code += [ln.split("//")[0] for ln in f.read().splitlines()]
    steps = {"DESC_STEP_CONSTANT": 0, "DESC_STEP_HYBRID": 2}
    with open(os.path.join(ROOT, "include", "desc_amd.h")) as f:
        hdr = f.read()
    for k, v in steps.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (k, v), hdr), k
    # a sweep kernel is named only where an entry is made, and launched only through an entry's pointer
    naming = [ln for ln in code if re.search(r"\bk_sweep(_node|_small|_band|_big)?<[^%\"]", ln)]          # ("k_sweep<%d,": a name's format)
    assert len(naming) == 5 and all(re.search(r"^constexpr SweepInst<.*> \w+_inst\(\) \{ return ", ln) for ln in naming), naming
    assert not [ln for ln in code if re.search(r"hipLaunchKernelGGL\(\(*k_sweep", ln)]
    entries = re.findall(r"\b(gather|big|small|node|band)_inst(?:<([^>]*)>)?\(\)(?! \{)", "\n".join(code))
    assert len(entries) == len(set(entries)), entries          # every argument tuple in exactly one table entry
    names = set()
    for family, args in entries:
        a = [str(steps.get(x.strip(), x.strip())) for x in args.split(",")]
        for s in steps.values():
            if family == "gather":
                names.add("k_sweep<%s,%d>" % (a[0], s))
            elif family == "big":
                names.add("k_sweep_big<%d>" % s)
            elif family == "small":
                names.add("k_sweep_small<%s,%d>" % (a[0], s))
            elif family == "node":
                names.update("k_sweep_node<%s,%s,%d>%s" % (a[0], a[1], s, suffix) for suffix in ("", " sharded"))
        if family == "band":
            names.update("k_sweep_band<%s,%s,%s,%s,%s>" % (*a, xt) for xt in ("one-rank", "XT"))
    return names


def test_table_covers_every_instance(oracle):
    """The case table names every sweep instance the sweep units can launch, and nothing else; every case's graph gives exactly T cycles
    in its longest segment (oracle structure)."""
    names = _instances()
    assert len(names) == 52, sorted(names)
    table = {c[4] for c in CASES}
    assert table == names, (sorted(names - table), sorted(table - names))
    assert len({_case_id(c) for c in CASES}) == len(CASES)
    for T in sorted({c[1] for c in CASES}):
        assert T in GRAPHS or T - 1 in GRAPHS, T
        st = oracle.build_structure(*_graph(_base(T))[1:4], seed=0, n_sample_min=T)
        assert int(np.diff(st["cum_ind"]).max()) == T == st["n_sample"], T
    # both sides of every size edge are run, in every layout the edge applies to
    for layout in ("gather", "node", "band"):
        ts = {c[1] for c in CASES if c[0] == layout}
        for edge in (16, 32, 64, 128) if layout != "gather" else (16, 32, 64):
            assert edge in ts and edge + 1 in ts, (layout, edge)
    ts = {c[1] for c in CASES if c[0] == "auto"}
    assert {16, 17, 32, 33, 64, 65, 256, 257} <= ts


# ------------------------------------------------------------------------------------------------------------------ GPU cases
def _bands_env(layout, T):
    """~24 bands, so that every emulated rank gets a range of them (one band by default on graphs this small): the band sweep's LDS
    budget of a band (DESC_DEBUG_ROW_CAP), the node layout's nodes per band (DESC_DEBUG_BAND)."""
    n, p = GRAPHS[_base(T)]
    return dict(DESC_DEBUG_ROW_CAP=str(max(64, int(n * n * p / 24)))) if layout.startswith("band") else dict(DESC_DEBUG_BAND=str(max(1, n // 24)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_sweep_instance_matches_oracle(lib, oracle, case, monkeypatch):
    layout, T, step, world, name = case
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)
    if world > 1:
        for k, v in _bands_env(layout, T).items():
            monkeypatch.setenv(k, v)
    mo, nn, ii, jj, rij = _graph(_base(T))
    st, S0, ref = _reference(oracle, T, step)
    assert int(np.diff(st["cum_ind"]).max()) == T
    p = c_params(_iters(T), seed=0, **STEPS[step])
    # Adam divides by sqrt(v) + 1e-8: rounding differences are amplified where v ~ 0 (test_gpu_parity.py::test_step_plugins)
    tol = 1e-9 if step == "adam" else TOL
    prob = lib.ProblemArrays(nn, ii, jj, rij)
    if world == 1:
        dst = lib.Structure.build(prob, T, 0, lib.BUILD_HOST, 0)
        arrays = dst.arrays()
        solver = lib.Solver(prob, dst, 0)
        try:
            assert solver.max_cnt == T
            s0 = solver.s0()
            out = solver.run(p, want_w=True)
            last = solver.last_sweep()
        finally:
            solver.destroy(); dst.free()
        assert last == name
        assert_structure_equal(arrays, st)
        assert np.abs(s0 - S0).max() <= 1e-14
        assert out["iters_run"] == ref["iters_run"]
        assert np.abs(out["S_vec"] - ref["S_vec"]).max() <= tol
        assert np.abs(out["w"] - ref["w"]).max() <= tol
        assert np.allclose(out["obj"], ref["obj"], rtol=1e-12, atol=1e-9)
        assert np.allclose(out["avg"], ref["avg"], rtol=1e-9, atol=1e-14)
        return
    outs, segs = emulate_sharded(lib, nn, ii, jj, rij, p, world, where=lib.BUILD_DEVICE, nmin=T)
    assert segs[0][0] == 0 and segs[-1][1] == st["m_pos"] and segs[-1][3] == st["m_cycle"]
    busy = [sg[1] > sg[0] for sg in segs]
    assert sum(busy) >= 2, segs
    for out, b in zip(outs, busy):
        if b:
            assert out["last_sweep"] == name, (out["last_sweep"], segs)
        assert out["iters_run"] == ref["iters_run"]
        assert np.abs(out["S_vec"] - ref["S_vec"]).max() <= tol
        assert np.allclose(out["obj"], ref["obj"], rtol=1e-12, atol=1e-9)
        assert np.allclose(out["avg"], ref["avg"], rtol=1e-9, atol=1e-14)
    for out in outs[1:]:
        assert np.array_equal(out["S_vec"], outs[0]["S_vec"]) and np.array_equal(out["obj"], outs[0]["obj"])
    if "k_sweep_band" in name:
        # ... and bitwise what ONE rank computes with the same kernel shape (fixed-point mirror sums: no order dependence)
        dst = lib.Structure.build(prob, T, 0, lib.BUILD_DEVICE, 0)
        one = run_unsharded(lib, prob, dst, p)
        dst.free()
        assert one["last_sweep"] == name.replace(",XT>", ",one-rank>")
        assert one["iters_run"] == outs[0]["iters_run"]
        assert np.array_equal(one["S_vec"], outs[0]["S_vec"])

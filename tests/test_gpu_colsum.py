"""GPU tests of the mirror column sums (k_colsum_node, desc_amd/csrc/pgd.hip; DESC_PGD.m:185-191) on their own: the 64-bit fixed-point
T of every CSR slot, bit for bit against the integer reference of tests/colsum_cases.py -- per rank (partial sums), added over the ranks,
and after the reduce-scatter -- for every case, weight state, number of ranks and dispatch switch of the table there.  No tolerance
anywhere: everything is np.array_equal on int64.

T comes out of the library through what exists: a HipShard binds a torch int64 tensor T, colsum() writes the rank's partial sums into it
through xpos (with one rank too: the piecewise protocol has no exchange stream, so it never takes the CSR-direct path).  The weights the
sums are taken of: 1 / cnt in the `uniform` state; otherwise downloaded from the one-rank run of the same problem, parameters and
environment, after asserting that every rank of the sharded run holds that run's S_vec bit for bit (DESC_DEBUG_VARIANT=3 throughout, as
tests/test_gpu_sharded.py::test_sharded_band_sweep_emulated).

What the handles reported on an MI355X when this file was written (every test prints its own lines: pytest -s).  cl = lanes per
segment by rule (per rank: a rank's own average run decides); long/nodes = nodes with a workgroup each / nodes visited, per rank;
rounds = rounds of colsum_walk the longest segment end takes at 16 / 8 lanes (both widths are forced where the table says so):

    case            fx_bits  cl by rule                 rounds 16/8  long/nodes per rank
    triangle          60     8                            1 / 1     w1 3/3
    K64               56     16                           2 / 4     w1 64/64; w2 64/64 46/46
    er40              57     8 (w3: 8 16 8)               1 / 2     w1 40/40; w2 40/40 29/29; w3 40/40 32/32 23/23         (forced 8, 16)
    er200             54     8                            1 / 2     w1 200/200; w3 200/200 160/160 112/112; w8 200 184 176 160 144 120 96 72, all long
    er60_full         56     16                           2 / 4     w1 60/60; w2 60/60 42/42                                (forced 8, 16)
    er150_full        54     16                           4 / 7     w1 150/150; w3 150/150 120/120 90/90                    (forced 8, 16)
    K258              53     16                           8 / 16    w1 258/258; w3 258/258 208/208 148/148                  (forced 8, 16)
    bridged150_60     56     16                           1 / 2     w1 210/210; w2 150/150 152/152
    hub1500_mid       51     8 (w8: ranks 5, 6: 16)       1 / 2     w1 1500/1500; w2 1/1498 1/839; w3 1/1485 1/1030 1/801;
                                                                    w8 1/1271 1/1122 1/985 1/818 0/283 1/801 0/0 0/800 (rank 6 owns nothing);
                                                                    DESC_DEBUG_COLSUM_SHORT=0: long = nodes on every rank

Checked once against kernels made wrong on purpose (values only): one round fewer at 16 lanes fails K258 alone; one segment fewer on the
wave-per-node path fails hub1500_mid on 2, 3, 8 ranks alone; truncation instead of round-to-nearest in the 8-lane instance fails er40 and
er200 (`distinct`, `collapsed`), hub1500_mid (every state) and the forced 8-lane runs of er60_full, er150_full and K258 -- the `uniform`
state of er40 and er200 cannot see it (tests/test_colsum_reference_host.py::test_where_the_rounding_mode_shows); a column index paired
with the neighbouring cycle of its segment in the 16-lane instance fails `distinct` and `collapsed` wherever 16 lanes run and passes
`uniform` -- which is what those two states are for."""
import contextlib
import os

import numpy as np
import pytest

from tests import colsum_cases as CC
from tests.helpers import c_params, csr, emulate_sharded, reduce_scatter_by_hand

pytestmark = pytest.mark.gpu

_slots = {}            # (case, state, switches, world) -> the ranks' T added up, per CSR slot: compared across switches and worlds


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _env_of(case, switches):
    nn, ii, jj, rij = CC.graph(case)
    env = {"DESC_DEBUG_VARIANT": "3"}
    if max(CC.CASES[case]["worlds"]) > 1:      # ~12-24 bands, so that every rank owns some (the library never cuts below the longest row)
        env["DESC_DEBUG_ROW_CAP"] = str(max(64, 2 * ii.shape[0] // 24))
    env.update({k: str(v) for k, v in switches.items()})
    return env


def _emulate(lib, case, state, world, want_w):
    """One emulated run of `world` ranks up to the state's weights, then the probe: T of every rank after colsum(), after a second
    colsum(), T_recv after the reduce-scatter done by hand, and what the handles say about their layout."""
    import torch
    cfg, step = CC.CASES[case], CC.step_of(case, state)
    nn, ii, jj, rij = CC.graph(case)
    rec = {}

    def probe(shards):
        assert not any(s.stopped() for s in shards)               # a stopped handle's colsum() returns at once
        for s in shards: s.colsum()                               # reads d_w[t_done & 1]: the current weights
        torch.cuda.current_stream().synchronize()
        rec["T"] = [s.T.cpu().numpy().copy() for s in shards]
        for s in shards: s.colsum()
        torch.cuda.current_stream().synchronize()
        rec["T_again"] = [s.T.cpu().numpy().copy() for s in shards]
        reduce_scatter_by_hand(shards)
        torch.cuda.current_stream().synchronize()
        rec["T_recv"] = [s.T_recv.cpu().numpy().copy() for s in shards]
        rec["stats"] = [s.solver.layout_stats() for s in shards]
        rec["layout"] = [s.solver.shard_layout() for s in shards]
        rec["info"] = [dict(t_part=int(s.info.t_part), xparts=int(s.info.xparts), t_len=int(s.info.t_len)) for s in shards]
        if want_w:
            rec["w"] = shards[0].solver.download(want_w=True)["w"].copy()

    p = c_params(step["iters"], lr=step["lr"], seed=cfg["seed"])
    outs, segs = emulate_sharded(lib, nn, ii, jj, rij, p, world, where=lib.BUILD_DEVICE if cfg["where"] == "device" else lib.BUILD_HOST,
                                 nmin=cfg["nmin"], probe=probe)
    assert all(o["iters_run"] == step["iters"] for o in outs)
    rec["S_vec"] = [o["S_vec"] for o in outs]
    rec["segs"] = segs
    return rec


def _check(lib, oracle, case, state, switches=None):
    """Every assertion on T for one case, state and set of switches, over the worlds of the case.  Returns {world: [layout_stats per rank]}."""
    switches = dict(switches or {})
    skey = tuple(sorted(switches.items()))
    cfg = CC.CASES[case]
    nn, ii, jj, rij = CC.graph(case)
    st = CC.structure(oracle, case)
    m, mp = ii.shape[0], st["m_pos"]
    max_deg = CC.max_degree(nn, ii, jj)
    fx = CC.fx_bits_of(max_deg)
    entries = int(np.count_nonzero(st["ikj"] >= 0) + np.count_nonzero(st["jki"] >= 0))
    rowptr, adj, adj_eid, row_of = csr(nn, ii, jj)
    seg_of_edge = np.full(m, -1, dtype=np.int64); seg_of_edge[st["pos_edge"][:mp]] = np.arange(mp)
    stats_by_world = {}
    with _environment(_env_of(case, switches)):
        one = _emulate(lib, case, state, 1, want_w=state != "uniform")
        # ---- the weights and the reference
        if state == "uniform":
            w = CC.uniform_weights(st)
        else:
            w = one.pop("w")
            assert w.shape == (st["m_cycle"],) and w.min() >= 0.0 and w.max() <= 1.0
        if state == "distinct":
            frac = CC.distinct_fraction(st, w)
            print("%s: %.4f %% of the contributing cycles carry a weight of their own in their segment" % (case, 100 * frac))
            assert frac >= 0.99, frac
        if state == "collapsed" and case != "triangle":
            assert np.count_nonzero(w == 0.0) > 0.5 * w.size       # mostly exact zeros
        q = CC.quantize(w, fx)
        T1, T2 = CC.mirror_sums(st, q)
        ref_slot = CC.per_slot(st, nn, ii, jj, T1, T2)
        print("%s %s %s: fx_bits %d, largest column sum %.3f" % (case, state, switches, fx, float(ref_slot.max()) * 2.0 ** -fx))
        for world in cfg["worlds"]:
            run = one if world == 1 else _emulate(lib, case, state, world, want_w=False)
            stats, lays, infos = run["stats"], run["layout"], run["info"]
            stats_by_world[world] = stats
            print("  world %d: colsum_cl %s, colsum_long / colsum_nodes %s, entries %s, segments %s" % (
                world, [s["colsum_cl"] for s in stats], ["%d/%d" % (s["colsum_long"], s["colsum_nodes"]) for s in stats],
                [s["colsum_entries"] for s in stats], [s["segments"] for s in stats]))
            for o in run["S_vec"]:                                 # the ranks hold the one-rank run's iterate: its w is theirs
                assert np.array_equal(o, one["S_vec"][0])
            assert all(s["colsum_fx_bits"] == fx for s in stats)
            assert sum(s["colsum_entries"] for s in stats) == entries
            assert sum(s["segments"] for s in stats) == mp
            xpos = lays[0]["xpos"].astype(np.int64)
            assert np.unique(xpos).size == 2 * m
            total = np.zeros(2 * m, dtype=np.int64)
            owned_all = np.zeros(mp, dtype=np.int64)
            for r in range(world):
                T, lay, info = run["T"][r], lays[r], infos[r]
                assert T.dtype == np.int64 and T.shape == (info["t_len"],) and np.array_equal(lay["xpos"], lays[0]["xpos"])
                # repeat call: nothing is left in an accumulator
                assert np.array_equal(run["T_again"][r], T)
                # ownership, from the rank's slot_ab: {slot (row i, column j), slot (row j, column i)} of its segments' edges
                sa, sb = lay["slot_ab"][:, 0].astype(np.int64), lay["slot_ab"][:, 1].astype(np.int64)
                assert sa.shape[0] == stats[r]["segments"]
                assert np.all(adj[sa] > row_of[sa]) and np.all(adj[sb] == row_of[sa]) and np.all(row_of[sb] == adj[sa]) and np.array_equal(adj_eid[sa], adj_eid[sb])
                segs_r = seg_of_edge[adj_eid[sa]]
                assert np.all(segs_r >= 0) and np.unique(segs_r).size == segs_r.size
                owned = np.zeros(mp, dtype=bool); owned[segs_r] = True
                owned_all += owned
                if world == 1:
                    part = ref_slot
                else:
                    P1, P2 = CC.mirror_sums(st, q, owned)
                    part = CC.per_slot(st, nn, ii, jj, P1, P2)
                got = T[xpos]
                bad = np.flatnonzero(got != part)
                assert bad.size == 0, "rank %d of %d: %d slots differ, first slot %d (row %d, column %d): %d units of 2^-%d" % (
                    r, world, bad.size, bad[0], row_of[bad[0]], adj[bad[0]], int(got[bad[0]] - part[bad[0]]), fx)
                rest = np.ones(T.shape[0], dtype=bool); rest[xpos] = False
                assert not T[rest].any()                           # every other entry of T stays 0
                total += got
            assert np.all(owned_all == 1)                          # every segment has exactly one owner
            assert np.array_equal(total, ref_slot)
            assert np.array_equal(total, one["T"][0][one["layout"][0]["xpos"].astype(np.int64)])      # = the one-rank T, each through its own xpos
            # after the reduce-scatter every rank holds the totals of its segments at xt, inside the exchange part of the segment
            for r in range(world):
                lay, info = lays[r], infos[r]
                if lay["slot_ab"].shape[0] == 0:
                    continue
                sa, sb = lay["slot_ab"][:, 0].astype(np.int64), lay["slot_ab"][:, 1].astype(np.int64)
                block = xpos[sa] // info["t_part"]
                assert np.all(block % world == r) and np.array_equal(block, xpos[sb] // info["t_part"])
                off = (block // world) * info["t_part"]
                segs_r = seg_of_edge[adj_eid[sa]]
                Tr = run["T_recv"][r]
                assert Tr.shape == (info["xparts"] * info["t_part"],)
                assert np.array_equal(Tr[off + lay["xt"][:, 0]], T1[segs_r]) and np.array_equal(Tr[off + lay["xt"][:, 1]], T2[segs_r])
            _slots[(case, state, skey, world)] = total
            # which path ran
            for s in stats:
                if "DESC_DEBUG_COLSUM_CL" in switches:
                    assert s["colsum_cl"] == int(switches["DESC_DEBUG_COLSUM_CL"])
                else:                                              # setup_node: 8 lanes exactly when the rank's average run is <= 10.5 (and it has segments)
                    by_rule = 8 if s["segments"] > 0 and 0 < s["colsum_entries"] / (2.0 * s["segments"]) <= 10.5 else 16
                    assert s["colsum_cl"] == by_rule, s
                assert 0 <= s["colsum_long"] <= s["colsum_nodes"] <= nn
                if max_deg < 4 * CC.COLSUM_SHORT - 1 or world == 1:
                    assert s["colsum_long"] == s["colsum_nodes"]  # the wave-per-node path is not eligible
            if world == 1:
                assert stats[0]["colsum_nodes"] == nn and stats[0]["colsum_entries"] == entries
    return stats_by_world


ALL = [(c, s) for c in CC.CASES for s in CC.states_of(c)]


@pytest.mark.parametrize("case,state", ALL, ids=["%s-%s" % cs for cs in ALL])
def test_column_sums_bit_for_bit(lib, oracle, case, state):
    """Every case and weight state, default dispatch, over the worlds of the case."""
    stats = _check(lib, oracle, case, state)
    if case == "triangle":
        one = _slots[(case, state, (), 1)]
        assert np.all(one == 1 << 60)                              # one cycle per segment, weight 1: every column is 2^60
    if case in ("er40", "er200", "hub1500_mid"):
        assert all(s["colsum_cl"] == 8 for s in stats[1])
    if case in ("K64", "er60_full", "er150_full", "K258", "bridged150_60"):
        assert all(s["colsum_cl"] == 16 for s in stats[1])


LANES = [(c, s) for c in ("er40", "er60_full", "er150_full", "K258") for s in CC.states_of(c)]


@pytest.mark.parametrize("cl", [8, 16])
@pytest.mark.parametrize("case,state", LANES, ids=["%s-%s" % cs for cs in LANES])
def test_lane_width_forced(lib, oracle, case, state, cl):
    """DESC_DEBUG_COLSUM_CL: the 8- and the 16-lane instance of k_colsum_node on the same weights (segment ends of up to 256 contributing
    cycles: up to 16 and 8 rounds of colsum_walk).  Both equal the reference; the handles report the forced width."""
    stats = _check(lib, oracle, case, state, {"DESC_DEBUG_COLSUM_CL": cl})
    assert all(s["colsum_cl"] == cl for ss in stats.values() for s in ss)


@pytest.mark.parametrize("state", sorted(CC.STATES))
@pytest.mark.parametrize("case", ["er40", "hub1500_mid"])
def test_visiting_order(lib, oracle, case, state):
    """DESC_DEBUG_NODE_ORDER 0 ascending, 1 longest row first, 2 reverse (default), 3 hashed: the same T whatever order the nodes are visited in."""
    for mode in (0, 1, 2, 3):
        _check(lib, oracle, case, state, {"DESC_DEBUG_NODE_ORDER": mode})
    for world in CC.CASES[case]["worlds"]:
        base = _slots[(case, state, (("DESC_DEBUG_NODE_ORDER", 0),), world)]
        for mode in (1, 2, 3):
            assert np.array_equal(_slots[(case, state, (("DESC_DEBUG_NODE_ORDER", mode),), world)], base)


@pytest.mark.parametrize("state", sorted(CC.STATES))
def test_short_run_path(lib, oracle, state):
    """hub1500_mid on 2, 3 and 8 ranks: by default the rows with at most 128 owned segments are summed by a wave each (wave-private columns, no
    barrier) -- colsum_long < colsum_nodes on at least one rank; DESC_DEBUG_COLSUM_SHORT=0 gives every node a workgroup.  The same T."""
    case = "hub1500_mid"
    dflt = _check(lib, oracle, case, state)
    off = _check(lib, oracle, case, state, {"DESC_DEBUG_COLSUM_SHORT": 0})
    for world in (2, 3, 8):
        assert any(s["colsum_long"] < s["colsum_nodes"] for s in dflt[world]), dflt[world]
        assert all(s["colsum_long"] == s["colsum_nodes"] for s in off[world]), off[world]
        assert [s["colsum_nodes"] for s in off[world]] == [s["colsum_nodes"] for s in dflt[world]]
        assert np.array_equal(_slots[(case, state, (), world)], _slots[(case, state, (("DESC_DEBUG_COLSUM_SHORT", 0),), world)])

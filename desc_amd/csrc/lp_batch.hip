// linprog_sij's LP for many small problems at once (desc_lp_batch_*): the row of a Monte-Carlo study that lp.hip solves one problem per
// call -- thousands of PDHG steps of two launches each, ten more launches and two blocking read-backs per check, a few microseconds of
// work behind every launch on a 100-node graph.  Here the variables and cycles of all B problems lie behind one another and every launch
// of the loop is shared by the batch.
//
// Layout.  Problem b's variables (its edges with a 3-cycle, ascending) are the batch-global variables var_off[b] .. var_off[b + 1); cycle t
// of its variable l is the batch-global cycle row_off[b] + l * nsample_b + t, with its two LP rows in y[2 c], y[2 c + 1].  nsample is per
// problem (the given value, or the rule of linprog_sij.m:43 evaluated for that problem alone).  va / vb (the variables of the edges ik and
// jk of a cycle) and the incidence lists hold batch-global ids, so the passes of lp_math.h index the batch's arrays directly.
//
// create (nothing here depends on tol, max_iter, check_every or restart):
//   host                 validation, the per-problem CSR (batch_csr.h), the codegree of every edge by a merge of the two sorted CSR rows ->
//                        the variables, m_pos, nsample, the offsets, the virtual grids and the two workgroup tables
//   k_lpb_samples        one wave per variable: the common neighbours in ascending k (cemp_batch.h: the CEMP batch sampler's text and
//                        its cap of 4096 neighbours per node), sample t = staged[desc_sample_key(seed_b, local edge id, t) mod codeg]
//                        -- cemp_build's rule --, k, va, vb and S0Mat (cemp_math.h)
//   k_lp_count, k_lpb_scan (one workgroup per problem: k_lp_scan's chunks over that problem's counts), k_lp_fill, k_lp_sort
//                        the transposed incidence of the whole batch in four launches; every list ascending
//
// run: desc_lp_sij_run_dev's loop for every problem in lockstep.
//   per step             k_lpb_col, k_lpb_row over the workgroup tables.  A table entry is {problem, block inside the problem}: problem b
//                        owns ncol_b = grid_for(m_pos_b, 2048, 16) consecutive entries of the column table and nrow_b = grid_for(m_pos_b,
//                        4096, nsample_b <= 32 ? 8 : 4) of the row table -- the grids lp.hip launches for it alone --, and a workgroup runs
//                        lp_math.h's pass as block blk of nblk.  So the first variable of an entry is 16 blk (8 or 4 blk in the row table),
//                        its count 16 (8, 4), the stride of a second pass the problem's own grid; an entry never spans two problems.
//                        32 or 64 lanes per variable is a workgroup-uniform branch on the problem's nsample.
//   per check            k_lpb_eval_row, k_lpb_eval_col (block partials at the problem's offset), k_lpb_final (one workgroup of 256 per
//                        problem: lp_eval_final) for the iterate; with restart k_lpb_average and the same three for the average;
//                        k_lpb_decide: per problem lp_decide (lp_math.h, the text the host runs in lp.hip) on the two records, the
//                        restart rule's memory, the stop -- which fixes the returned point, sets the problem's stop flag and decrements
//                        the word "problems still running", all the host reads per check --; k_lpb_apply: the copy or clear of a restart.
// A workgroup whose problem has stopped returns at once: nothing of the problem is written again.
//
// Why a result does not depend on the batch.  Every sum of a problem is taken over its own virtual grid in that grid's block order, the
// arithmetic is lp_math.h's, the decisions are lp_decide's on the same doubles: problem b's S, y and record are bit for bit what
// desc_lp_sij_run_dev computes for it alone.  No floating-point atomics; integer atomics in k_lp_count / k_lp_fill (their order is undone
// by k_lp_sort) and on the running count.  Every loop is bounded by a size or by max_iter; nothing spins on memory.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>

#include "cemp_batch.h"
#include "cemp_math.h"
#include "lp_math.h"

namespace desc {
namespace {

struct LbProb {                       // one problem of the batch as the kernels see it
    int32_t mp, nsample;              // variables, samples per variable
    int32_t var_off, row_off;         // first batch-global variable, first batch-global cycle
    int32_t ncol, nrow;               // the virtual grids of the column and the row half
    int32_t pcol_off, prow_off;       // first block partial (a pair of doubles) of either half
    int32_t node_off, edge_off;
    uint64_t seed;
};
struct LbState {                      // the loop of one problem: lp_decide's memory and what the stop fixed
    LpLoop loop;
    int32_t it_restart;               // step of the last restart: cnt = it - it_restart
    int32_t iters, converged, fin_avg, action;
    LpRec fin;
};
struct LbTab { int32_t prob, blk; };

struct LbArgs {
    const LbProb* prob;
    const LbTab *col_tab, *row_tab;
    const int32_t *vprob, *vedge;     // variable -> problem, local edge id
    const int32_t* poe;               // batch-global edge -> batch-global variable (-1: no cycle)
    const int32_t *ii, *jj, *rowptr, *adj, *adj_eid;      // as CbArgs (cemp_batch.h)
    const double* rij;
    int32_t *kk, *va, *vb, *ptr, *list;                   // per cycle: the third node (local) and the two other variables; the incidence
    double *S0, *tau0;
    double *x, *xbar, *own, *ownt, *z, *zt, *y, *xs, *ys, *xa, *ya, *part_row, *part_col;
    LpRec *rec_cur, *rec_avg;
    LbState* state;
    int32_t *stop, *running;
    double* s_vec;
    int32_t lds_cap;
};

// ---- create
__global__ __launch_bounds__(256) void k_lpb_samples(LbArgs a, int MP) {
    extern __shared__ uint32_t lb_stage[];             // per wave: lds_cap packed positions of the common neighbours (cemp_batch.h)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t* st = lb_stage + (size_t)wv * a.lds_cap;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t v64 = wid; v64 < MP; v64 += nw) {
        const int v = __builtin_amdgcn_readfirstlane((int)v64);
        const int b = uniform_load(a.vprob, v), e = uniform_load(a.vedge, v);
        const LbProb pd = a.prob[b];
        const int g = pd.edge_off + e;
        const int i = uniform_load(a.ii, g), j = uniform_load(a.jj, g);
        const int32_t* rp = a.rowptr + pd.node_off + b;
        const int32_t* adj = a.adj + 2 * (int64_t)pd.edge_off;
        const int32_t* eid = a.adj_eid + 2 * (int64_t)pd.edge_off;
        const int ri = uniform_load(rp, i), di = uniform_load(rp, i + 1) - ri;
        const int rj = uniform_load(rp, j), dj = uniform_load(rp, j + 1) - rj;
        const int cd = cb_common_neighbours(adj, ri, di, rj, dj, lane, a.lds_cap, st);
        if (cd == 0) continue;                                           // never: the host made a variable of an edge with a cycle only
        double A[9];
        load_block9(a.rij + 9 * (int64_t)g, A);
        const int64_t c0 = (int64_t)pd.row_off + (int64_t)(v - pd.var_off) * pd.nsample;
        for (int s = lane; s < pd.nsample; s += 64) {
            const uint32_t p = st[d_sample_key(pd.seed, (uint64_t)e, (uint64_t)s) % (uint64_t)cd];
            const int xi = (int)(p & 0xFFFFu), xj = (int)(p >> 16);
            const int k = adj[ri + xi];
            const int eki = pd.edge_off + eid[ri + xi], ejk = pd.edge_off + eid[rj + xj];
            double pb[9], pc[9];
            load_block9(a.rij + 9 * (int64_t)ejk, pb);
            load_block9(a.rij + 9 * (int64_t)eki, pc);
            a.kk[c0 + s] = k; a.va[c0 + s] = a.poe[eki]; a.vb[c0 + s] = a.poe[ejk];
            a.S0[c0 + s] = cemp_cycle_dist(A, pb, pc, !(j < k), !(k < i));
        }
        __builtin_amdgcn_wave_barrier();                                 // the staging area is reused by the wave's next variable
    }
}

// k_lp_scan for every problem: workgroup b scans the counts of problem b's variables; its lists start at entry 2 row_off[b] of the batch's
__global__ __launch_bounds__(1024) void k_lpb_scan(LbArgs a, int32_t* cnt, int last) {
    const int b = blockIdx.x;
    const LbProb pd = a.prob[b];
    if (pd.mp == 0) return;
    lp_scan_block(cnt + pd.var_off, a.ptr + pd.var_off, a.tau0 + pd.var_off, pd.mp, pd.nsample, 2 * (int64_t)pd.row_off, b == last);
}

// ---- the loop
template <bool AVG>
__global__ __launch_bounds__(256) void k_lpb_col(LbArgs a) {
    const LbTab t = a.col_tab[blockIdx.x];
    if (a.stop[t.prob]) return;
    const LbProb pd = a.prob[t.prob];
    lp_col_pass<AVG>(a.ptr, a.list, a.z, a.own, a.tau0, a.x, a.xbar, a.xs, pd.mp, t.blk, pd.ncol, pd.var_off);
}
template <bool AVG>
__global__ __launch_bounds__(256) void k_lpb_row(LbArgs a, double sigma) {
    const LbTab t = a.row_tab[blockIdx.x];
    if (a.stop[t.prob]) return;
    const LbProb pd = a.prob[t.prob];
    if (pd.nsample <= 32) lp_row_pass<32, AVG>(a.va, a.vb, a.S0, a.xbar, (double2*)a.y, (double2*)a.ys, a.z, a.own, sigma, pd.mp, pd.nsample, t.blk, pd.nrow, pd.var_off, pd.row_off);
    else lp_row_pass<64, AVG>(a.va, a.vb, a.S0, a.xbar, (double2*)a.y, (double2*)a.ys, a.z, a.own, sigma, pd.mp, pd.nsample, t.blk, pd.nrow, pd.var_off, pd.row_off);
}
// certificates of the point (x, y): z / own of y land in zt / ownt
__global__ __launch_bounds__(256) void k_lpb_eval_row(LbArgs a, const double* x, const double* y) {
    const LbTab t = a.row_tab[blockIdx.x];
    if (a.stop[t.prob]) return;
    const LbProb pd = a.prob[t.prob];
    double* part = a.part_row + 2 * ((int64_t)pd.prow_off + t.blk);
    if (pd.nsample <= 32) lp_eval_row_pass<32>(a.va, a.vb, a.S0, x, (const double2*)y, a.zt, a.ownt, part, pd.mp, pd.nsample, t.blk, pd.nrow, pd.var_off, pd.row_off);
    else lp_eval_row_pass<64>(a.va, a.vb, a.S0, x, (const double2*)y, a.zt, a.ownt, part, pd.mp, pd.nsample, t.blk, pd.nrow, pd.var_off, pd.row_off);
}
__global__ __launch_bounds__(256) void k_lpb_eval_col(LbArgs a, const double* x) {
    const LbTab t = a.col_tab[blockIdx.x];
    if (a.stop[t.prob]) return;
    const LbProb pd = a.prob[t.prob];
    lp_eval_col_pass(a.ptr, a.list, a.zt, a.ownt, x, a.part_col + 2 * ((int64_t)pd.pcol_off + t.blk), pd.mp, t.blk, pd.ncol, pd.var_off);
}
// one workgroup per problem over its partials, in its grids' block order
__global__ __launch_bounds__(256) void k_lpb_final(LbArgs a, LpRec* rec) {
    const int b = blockIdx.x;
    if (a.stop[b]) return;
    const LbProb pd = a.prob[b];
    lp_eval_final(a.part_row + 2 * (int64_t)pd.prow_off, pd.nrow, a.part_col + 2 * (int64_t)pd.pcol_off, pd.ncol, &rec[b]);
}
// the running averages since the problem's last restart
__global__ __launch_bounds__(256) void k_lpb_average(LbArgs a, int it) {
    const LbTab t = a.row_tab[blockIdx.x];
    if (a.stop[t.prob]) return;
    const LbProb pd = a.prob[t.prob];
    const double cnt = (double)(int64_t)(it - a.state[t.prob].it_restart);
    const int64_t first = (int64_t)t.blk * 256 + threadIdx.x, stride = (int64_t)pd.nrow * 256, ny = 2 * (int64_t)pd.mp * pd.nsample;
    for (int64_t u = first; u < pd.mp; u += stride) a.xa[pd.var_off + u] = lp_average(a.xs[pd.var_off + u], cnt);
    for (int64_t u = first; u < ny; u += stride) a.ya[2 * (int64_t)pd.row_off + u] = lp_average(a.ys[2 * (int64_t)pd.row_off + u], cnt);
}
// The decisions of a check, one thread per problem (lp.hip takes them on the host from the same records by the same lp_decide).
// final_only: no check ran (restart = 0 and tol = 0, or max_iter = 0): the record of the last iterate is the returned one.
__global__ __launch_bounds__(256) void k_lpb_decide(LbArgs a, int count, int it, int max_iter, double tol, int restart, int final_only) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= count || a.stop[b]) return;
    LbState& s = a.state[b];
    bool use_avg = false;
    int act = LP_CONTINUE;
    if (!final_only) {
        const LpRec none{};
        act = lp_decide(s.loop, a.rec_cur[b], restart ? a.rec_avg[b] : none, restart != 0, tol, (int64_t)(it - s.it_restart), it, max_iter, &use_avg);
    }
    if (final_only || act == LP_CONVERGED || it == max_iter) {          // the stop: the returned point and its record are fixed here
        s.fin = use_avg ? a.rec_avg[b] : a.rec_cur[b];
        s.fin_avg = use_avg ? 1 : 0; s.iters = it; s.converged = act == LP_CONVERGED ? 1 : 0; s.action = LP_CONTINUE;
        a.stop[b] = 1;
        atomicSub(a.running, 1);
        return;
    }
    s.action = act;
    if (act == LP_RESTART_AVG || act == LP_RESTART_CUR) s.it_restart = it;
}
// what a restart does to the problem's arrays: from the average, x, y <- the average and z, own <- those of the average's y (zt, ownt of
// its evaluation, the last of the check); from the iterate nothing moves.  Either way the running sums start again.
__global__ __launch_bounds__(256) void k_lpb_apply(LbArgs a) {
    const LbTab t = a.row_tab[blockIdx.x];
    if (a.stop[t.prob]) return;
    const int act = a.state[t.prob].action;
    if (act != LP_RESTART_AVG && act != LP_RESTART_CUR) return;
    const LbProb pd = a.prob[t.prob];
    const int64_t first = (int64_t)t.blk * 256 + threadIdx.x, stride = (int64_t)pd.nrow * 256, nc = (int64_t)pd.mp * pd.nsample;
    const int64_t v0 = pd.var_off, c0 = pd.row_off;
    if (act == LP_RESTART_AVG) {
        for (int64_t u = first; u < pd.mp; u += stride) { a.x[v0 + u] = a.xa[v0 + u]; a.own[v0 + u] = a.ownt[v0 + u]; a.xs[v0 + u] = 0.0; }
        for (int64_t u = first; u < nc; u += stride) a.z[c0 + u] = a.zt[c0 + u];
        for (int64_t u = first; u < 2 * nc; u += stride) { a.y[2 * c0 + u] = a.ya[2 * c0 + u]; a.ys[2 * c0 + u] = 0.0; }
    } else {
        for (int64_t u = first; u < pd.mp; u += stride) a.xs[v0 + u] = 0.0;
        for (int64_t u = first; u < 2 * nc; u += stride) a.ys[2 * c0 + u] = 0.0;
    }
}
__global__ __launch_bounds__(256) void k_lpb_set(double* p, int64_t count, double v) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < count; t += (int64_t)gridDim.x * 256) p[t] = v;
}
// S_vec of the variables from each problem's returned point (edges without a cycle keep the 1 of k_lpb_set, :104)
__global__ __launch_bounds__(256) void k_lpb_out(LbArgs a, int MP) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < MP; v += (int64_t)gridDim.x * 256) {
        const int b = a.vprob[v];
        const double* x = a.state[b].fin_avg ? a.xa : a.x;
        a.s_vec[a.prob[b].edge_off + a.vedge[v]] = lp_clip(x[v]);
    }
}

// What create decides on the host, before any device call (desc_lp_batch_plan returns it without a device).
struct LbPlan {
    hvec<int32_t> nsample, ncol, nrow;        // per problem
    hvec<int64_t> m_pos, var_off, row_off;    // per problem; the offsets count + 1
    hvec<int32_t> pos;                        // the variables: local edge ids, problem b's at var_off[b]
    int32_t max_deg = 0;
    int64_t MP = 0, MC = 0;
};

int lb_plan(const desc_problem* probs, int32_t count, const int32_t* nsample_in, BatchCsr* h, LbPlan& pl) {
    for (int32_t b = 0; b < count && nsample_in; ++b)
        if (nsample_in[b] < 0) return fail(DESC_ERR_INVALID, "problem %d: nsample = %d, need nsample >= 0 (0: the rule of linprog_sij.m:43)", b, (int)nsample_in[b]);
    int rc = batch_csr_host(probs, count, nullptr, h);
    if (rc) return rc;
    for (int32_t b = 0; b < count; ++b) {
        const int32_t* rp = h->rowptr.data() + h->node_off[(size_t)b] + b;
        for (int64_t v = 0; v < probs[b].n; ++v) {
            const int32_t d = rp[v + 1] - rp[v];
            if (d > CEMP_BATCH_MAX_DEGREE)
                return fail(DESC_ERR_INVALID, "problem %d: node %lld has %d neighbours, more than the %d the batched sampler stages per row: solve it with linprog_sij",
                            b, (long long)v, (int)d, CEMP_BATCH_MAX_DEGREE);
            pl.max_deg = std::max(pl.max_deg, d);
        }
    }
    const size_t B = (size_t)count;
    pl.nsample.assign(B, 0); pl.ncol.assign(B, 0); pl.nrow.assign(B, 0); pl.m_pos.assign(B, 0);
    pl.var_off.assign(B + 1, 0); pl.row_off.assign(B + 1, 0);
    // the codegree of every edge: the two CSR rows are ascending, a merge counts their common entries
    hvec<int32_t> codeg((size_t)h->M);
    for_each_problem(count, [&](int32_t b) {
        const int32_t* rp = h->rowptr.data() + h->node_off[(size_t)b] + b;
        const int32_t* adj = h->adj.data() + 2 * h->edge_off[(size_t)b];
        const int64_t eo = h->edge_off[(size_t)b], m = probs[b].m, n = probs[b].n;
        hvec<int64_t> hist((size_t)n + 1, 0);
        int64_t hp = 0;
        for (int64_t e = 0; e < m; ++e) {
            const int32_t i = h->ii[(size_t)(eo + e)], j = h->jj[(size_t)(eo + e)];
            int32_t p = rp[i], q = rp[j], c = 0;
            const int32_t pe = rp[i + 1], qe = rp[j + 1];
            while (p < pe && q < qe) {
                const int32_t u = adj[p], w = adj[q];
                if (u == w) { ++c; ++p; ++q; } else if (u < w) ++p; else ++q;
            }
            codeg[(size_t)(eo + e)] = c;
            ++hist[(size_t)c];
            hp += c > 0;
        }
        pl.m_pos[(size_t)b] = hp;
        int32_t ns = nsample_in ? nsample_in[b] : 0;
        if (ns <= 0) {                                                   // linprog_sij.m:43 for this problem alone, as build_cemp_samples_device
            ns = 30;                                                     // median([]) = NaN, max(NaN, 30) = 30
            if (hp > 0) {
                auto kth = [&](int64_t r) {                              // r-th smallest positive codegree, 0-based
                    int64_t acc = 0;
                    for (int64_t c = 1; c <= n; ++c) { acc += hist[(size_t)c]; if (acc > r) return (double)c; }
                    return (double)n;
                };
                const double med = (hp & 1) ? kth(hp / 2) : 0.5 * (kth(hp / 2 - 1) + kth(hp / 2));     // MATLAB median
                ns = std::max(30, (int32_t)std::ceil(med / 4.0));
            }
        }
        pl.nsample[(size_t)b] = ns;
    });
    for (size_t b = 0; b < B; ++b) {
        const int64_t mp = pl.m_pos[b];
        pl.var_off[b + 1] = pl.var_off[b] + mp;
        pl.row_off[b + 1] = pl.row_off[b] + mp * pl.nsample[b];
        if (2 * pl.row_off[b + 1] >= (1ll << 31))
            return fail(DESC_ERR_TOO_LARGE, "problems 0 to %d hold %lld LP rows (2 * m_pos * nsample each): the batch exceeds 2^31, split the batch", (int)b,
                        (long long)(2 * pl.row_off[b + 1]));
        if (mp) {
            pl.ncol[b] = grid_for(mp, 2048, 16);
            pl.nrow[b] = grid_for(mp, 4096, pl.nsample[b] <= 32 ? 8 : 4);
        }
    }
    pl.MP = pl.var_off[B]; pl.MC = pl.row_off[B];
    pl.pos.resize((size_t)pl.MP);
    for (size_t b = 0; b < B; ++b) {
        size_t v = (size_t)pl.var_off[b];
        const int64_t eo = h->edge_off[b], m = probs[b].m;
        for (int64_t e = 0; e < m; ++e) if (codeg[(size_t)(eo + e)] > 0) pl.pos[v++] = (int32_t)e;
    }
    return DESC_OK;
}

}  // namespace
}  // namespace desc

using namespace desc;

struct desc_lp_batch : desc::BatchCsr, desc::BatchDevice {
    LbPlan plan;
    LbArgs a{};
    hvec<uint64_t> seeds;
    int64_t n_col_tab = 0, n_row_tab = 0;
    int32_t live = 0;                         // problems with a variable
    bool avg_ready = false;                   // the arrays of the running averages (first run with restart)
    double ms_build = 0;
};

namespace {

int lb_create(const desc_problem* probs, int32_t count, const int32_t* nsample_in, const uint64_t* seeds, int32_t device, desc_lp_batch* h) {
    auto t0 = std::chrono::steady_clock::now();
    LbPlan& pl = h->plan;
    int rc = lb_plan(probs, count, nsample_in, h, pl);
    if (rc) return rc;
    const size_t B = (size_t)count, M = (size_t)h->M, MP = (size_t)pl.MP, MC = (size_t)pl.MC;
    h->seeds.assign(B, 0);
    for (size_t b = 0; b < B && seeds; ++b) h->seeds[b] = seeds[b];
    // the kernels' view of every problem, the two workgroup tables, variable -> problem and edge -> variable
    hvec<LbProb> pr(B);
    hvec<LbTab> col_tab, row_tab;
    hvec<int32_t> vprob(MP), poe(M, -1);
    int64_t pcol = 0, prow = 0;
    int last = -1;
    for (size_t b = 0; b < B; ++b) {
        const int64_t mp = pl.m_pos[b];
        pr[b] = LbProb{(int32_t)mp, pl.nsample[b], (int32_t)pl.var_off[b], (int32_t)pl.row_off[b], pl.ncol[b], pl.nrow[b], (int32_t)pcol, (int32_t)prow,
                       (int32_t)h->node_off[b], (int32_t)h->edge_off[b], h->seeds[b]};
        for (int32_t k = 0; k < pl.ncol[b]; ++k) col_tab.push_back(LbTab{(int32_t)b, k});
        for (int32_t k = 0; k < pl.nrow[b]; ++k) row_tab.push_back(LbTab{(int32_t)b, k});
        pcol += pl.ncol[b]; prow += pl.nrow[b];
        for (int64_t l = 0; l < mp; ++l) {
            const size_t v = (size_t)(pl.var_off[b] + l);
            vprob[v] = (int32_t)b;
            poe[(size_t)h->edge_off[b] + (size_t)pl.pos[v]] = (int32_t)v;
        }
        if (mp) { last = (int)b; ++h->live; }
    }
    h->n_col_tab = (int64_t)col_tab.size(); h->n_row_tab = (int64_t)row_tab.size();
    h->ms_structure = ms_since(t0);
    if (count == 0) return DESC_OK;

    if ((rc = h->open(device, "the batched linprog_sij"))) return rc;     // nothing above touched the device
    auto t1 = std::chrono::steady_clock::now();
    const hvec<double> rij = stage_rotations(probs, count, h->edge_off);
    LbArgs& a = h->a;
    if ((rc = h->upload(&a.prob, pr.data(), B)) || (rc = h->upload(&a.col_tab, col_tab.data(), col_tab.size())) ||
        (rc = h->upload(&a.row_tab, row_tab.data(), row_tab.size())) || (rc = h->upload(&a.vprob, vprob.data(), MP)) ||
        (rc = h->upload(&a.vedge, pl.pos.data(), MP)) || (rc = h->upload(&a.poe, poe.data(), M)) ||
        (rc = h->upload(&a.ii, h->ii.data(), M)) || (rc = h->upload(&a.jj, h->jj.data(), M)) ||
        (rc = h->upload(&a.rowptr, h->rowptr.data(), h->rowptr.size())) || (rc = h->upload(&a.adj, h->adj.data(), 2 * M)) ||
        (rc = h->upload(&a.adj_eid, h->adj_eid.data(), 2 * M)) || (rc = h->upload(&a.rij, rij.data(), 9 * M))) return rc;
    DevArena& D = h->mem;
    if ((rc = D.alloc(&a.kk, MC)) || (rc = D.alloc(&a.va, MC)) || (rc = D.alloc(&a.vb, MC)) || (rc = D.alloc(&a.S0, MC)) || (rc = D.alloc(&a.ptr, MP + 1)) ||
        (rc = D.alloc(&a.list, 2 * MC)) || (rc = D.alloc(&a.tau0, MP)) ||
        (rc = D.alloc(&a.x, MP)) || (rc = D.alloc(&a.xbar, MP)) || (rc = D.alloc(&a.own, MP)) || (rc = D.alloc(&a.ownt, MP)) || (rc = D.alloc(&a.z, MC)) ||
        (rc = D.alloc(&a.zt, MC)) || (rc = D.alloc(&a.y, 2 * MC)) || (rc = D.alloc(&a.part_row, 2 * (size_t)prow)) || (rc = D.alloc(&a.part_col, 2 * (size_t)pcol)) ||
        (rc = D.alloc(&a.rec_cur, B)) || (rc = D.alloc(&a.state, B)) || (rc = D.alloc(&a.stop, B)) || (rc = D.alloc(&a.running, 1)) || (rc = D.alloc(&a.s_vec, M))) return rc;
    DESC_HIP(hipStreamSynchronize(h->stream));         // the staging vectors go out of scope below
    h->ms_upload = ms_since(t1);
    if (MP == 0) return DESC_OK;                        // no problem has a triangle: every LP is empty

    // ---- the samples, S0Mat and the transposed incidence of the whole batch
    auto t2 = std::chrono::steady_clock::now();
    a.lds_cap = std::max(64, (pl.max_deg + 63) / 64 * 64);              // the longest row bounds every codegree
    const size_t lds = (size_t)4 * (size_t)a.lds_cap * sizeof(uint32_t);
    if (lds > 64 * 1024) return fail(DESC_ERR_STATE, "LDS budget exceeded (%zu bytes)", lds);
    hipLaunchKernelGGL(k_lpb_samples, dim3((unsigned)grid_for((int64_t)MP, 8192, 4)), dim3(256), lds, h->stream, a, (int)MP);
    DevArena T;                                         // scratch of the incidence builder
    int32_t *d_cnt, *d_list0;
    if ((rc = T.alloc(&d_cnt, MP)) || (rc = T.alloc(&d_list0, 2 * MC))) return rc;
    DESC_HIP(hipMemsetAsync(d_cnt, 0, sizeof(int32_t) * MP, h->stream));
    const int cgrid = grid_for((int64_t)MC, 4096);
    hipLaunchKernelGGL(k_lp_count, dim3(cgrid), dim3(256), 0, h->stream, a.va, a.vb, d_cnt, (int64_t)MC);
    hipLaunchKernelGGL(k_lpb_scan, dim3((unsigned)count), dim3(1024), 0, h->stream, a, d_cnt, last);
    hipLaunchKernelGGL(k_lp_fill, dim3(cgrid), dim3(256), 0, h->stream, a.va, a.vb, a.ptr, d_cnt, d_list0, (int64_t)MC);
    hipLaunchKernelGGL(k_lp_sort, dim3((unsigned)std::min<int64_t>((int64_t)MP, 65536)), dim3(64), 0, h->stream, a.ptr, d_list0, a.list, (int64_t)MP);
    DESC_HIP(hipGetLastError());
    DESC_HIP(hipStreamSynchronize(h->stream));          // T is freed below
    h->ms_build = ms_since(t2);
    return DESC_OK;
}

int lb_run(desc_lp_batch* h, const desc_lp_params* params, double* s_vec, double* y_out, desc_lp_info* infos, desc_lp_batch_timings* tm) {
    auto t0 = std::chrono::steady_clock::now();
    if (tm) { tm->ms_structure = h->ms_structure; tm->ms_upload = h->ms_upload; tm->ms_build = h->ms_build; tm->ms_loop = 0; tm->ms_total = 0; }
    desc_lp_params P;
    desc_lp_params_default(&P);
    if (params) P = *params;
    if (P.max_iter < 0 || P.check_every < 0 || !(P.tol >= 0.0)) return fail(DESC_ERR_INVALID, "need max_iter >= 0, check_every >= 0, tol >= 0");
    if (P.check_every == 0) P.check_every = 64;
    if (h->count == 0) { if (tm) tm->ms_total = ms_since(t0); return DESC_OK; }
    if (!s_vec || !infos) return fail(DESC_ERR_INVALID, "s_vec or infos is NULL");
    const LbPlan& pl = h->plan;
    const size_t B = (size_t)h->count, M = (size_t)h->M, MP = (size_t)pl.MP, MC = (size_t)pl.MC;
    const bool restart = P.restart != 0, checks = restart || P.tol > 0.0;
    int rc = DESC_OK;
    DESC_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    LbArgs& a = h->a;
    if (restart && !h->avg_ready && MP) {
        if ((rc = h->mem.alloc(&a.xs, MP)) || (rc = h->mem.alloc(&a.ys, 2 * MC)) || (rc = h->mem.alloc(&a.xa, MP)) || (rc = h->mem.alloc(&a.ya, 2 * MC)) ||
            (rc = h->mem.alloc(&a.rec_avg, B))) return rc;
        h->avg_ready = true;
    }
    // ---- the start: x = 0, y = 0, every problem with a variable running
    hvec<LbState> states(B);
    hvec<int32_t> stop(B);
    for (size_t b = 0; b < B; ++b) {
        states[b] = LbState{};
        const bool empty = pl.m_pos[b] == 0;                             // no triangle: the empty LP, S_vec = 1, solved before the first step
        states[b].converged = empty ? 1 : 0;
        stop[b] = empty ? 1 : 0;
    }
    int32_t running = h->live;
    hipLaunchKernelGGL(k_lpb_set, dim3(grid_for((int64_t)M, 1024)), dim3(256), 0, st, a.s_vec, (int64_t)M, 1.0);      // :104
    if (MP) {
        DESC_HIP(hipMemcpyAsync(a.state, states.data(), sizeof(LbState) * B, hipMemcpyHostToDevice, st));
        DESC_HIP(hipMemcpyAsync(a.stop, stop.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, st));
        DESC_HIP(hipMemcpyAsync(a.running, &running, sizeof(int32_t), hipMemcpyHostToDevice, st));
        for (double* q : {a.x, a.xbar, a.own, restart ? a.xs : nullptr}) if (q) DESC_HIP(hipMemsetAsync(q, 0, sizeof(double) * MP, st));
        DESC_HIP(hipMemsetAsync(a.z, 0, sizeof(double) * MC, st));
        for (double* q : {a.y, restart ? a.ys : nullptr}) if (q) DESC_HIP(hipMemsetAsync(q, 0, sizeof(double) * 2 * MC, st));
        DESC_HIP(hipStreamSynchronize(st));            // states / stop / running are host vectors of this frame: uploaded before the loop reads back
    }
    const dim3 gcol((unsigned)h->n_col_tab), grow((unsigned)h->n_row_tab), gb((unsigned)B), gdec((unsigned)((B + 255) / 256)), blk(256);
    auto evaluate = [&](const double* x, const double* y, LpRec* rec) {
        hipLaunchKernelGGL(k_lpb_eval_row, grow, blk, 0, st, a, x, y);
        hipLaunchKernelGGL(k_lpb_eval_col, gcol, blk, 0, st, a, x);
        hipLaunchKernelGGL(k_lpb_final, gb, blk, 0, st, a, rec);
    };
    int it = 0;
    const double sigma = 1.0 / 3.0;
    while (MP && running > 0 && it < P.max_iter) {
        ++it;
        if (restart) { hipLaunchKernelGGL(k_lpb_col<true>, gcol, blk, 0, st, a); hipLaunchKernelGGL(k_lpb_row<true>, grow, blk, 0, st, a, sigma); }
        else { hipLaunchKernelGGL(k_lpb_col<false>, gcol, blk, 0, st, a); hipLaunchKernelGGL(k_lpb_row<false>, grow, blk, 0, st, a, sigma); }
        if (!checks || (it % P.check_every != 0 && it != P.max_iter)) continue;
        evaluate(a.x, a.y, a.rec_cur);
        if (restart) {
            hipLaunchKernelGGL(k_lpb_average, grow, blk, 0, st, a, it);
            evaluate(a.xa, a.ya, a.rec_avg);                             // last: zt / ownt belong to the average
        }
        hipLaunchKernelGGL(k_lpb_decide, gdec, blk, 0, st, a, (int)B, it, (int)P.max_iter, P.tol, restart ? 1 : 0, 0);
        if (restart) hipLaunchKernelGGL(k_lpb_apply, grow, blk, 0, st, a);
        DESC_HIP(hipGetLastError());
        DESC_HIP(hipMemcpyAsync(&running, a.running, sizeof(int32_t), hipMemcpyDeviceToHost, st));      // all the host reads per check
        DESC_HIP(hipStreamSynchronize(st));
    }
    if (MP && running > 0) {                            // no check fixed a record: max_iter = 0, or restart = 0 with tol = 0
        evaluate(a.x, a.y, a.rec_cur);
        hipLaunchKernelGGL(k_lpb_decide, gdec, blk, 0, st, a, (int)B, it, (int)P.max_iter, P.tol, 0, 1);
    }
    if (MP) {
        hipLaunchKernelGGL(k_lpb_out, dim3(grid_for((int64_t)MP, 1024)), blk, 0, st, a, (int)MP);
        DESC_HIP(hipGetLastError());
        DESC_HIP(hipMemcpyAsync(states.data(), a.state, sizeof(LbState) * B, hipMemcpyDeviceToHost, st));
    }
    DESC_HIP(hipMemcpyAsync(s_vec, a.s_vec, sizeof(double) * M, hipMemcpyDeviceToHost, st));
    DESC_HIP(hipStreamSynchronize(st));
    if (y_out)
        for (size_t b = 0; b < B; ++b) {                                 // each problem's duals from its returned point
            const size_t off = 2 * (size_t)pl.row_off[b], len = 2 * (size_t)(pl.row_off[b + 1] - pl.row_off[b]);
            if (len) DESC_HIP(hipMemcpyAsync(y_out + off, (states[b].fin_avg ? a.ya : a.y) + off, sizeof(double) * len, hipMemcpyDeviceToHost, st));
        }
    DESC_HIP(hipStreamSynchronize(st));
    const double ms_loop = ms_since(t0);
    std::string late;
    for (size_t b = 0; b < B; ++b) {
        const LbState& s = states[b];
        desc_lp_info I{};
        I.nsample = pl.nsample[b]; I.m_pos = pl.m_pos[b]; I.rows = 2 * (pl.row_off[b + 1] - pl.row_off[b]);
        I.iters = s.iters; I.restarts = s.loop.restarts; I.converged = s.converged;
        I.viol = s.fin.viol; I.pobj = s.fin.P; I.dobj = lp_dual_obj(s.fin);
        I.ms_loop = ms_loop; I.ms_total = ms_loop;
        infos[b] = I;
        if (!s.converged && P.tol > 0.0) late += (late.empty() ? "" : ", ") + std::to_string(b);
    }
    if (!late.empty())
        fprintf(stderr, "[desc_amd] linprog_sij_batch: the LP solver stopped at max_iter = %d (tol %.1e) for problems %s: their S_vec is the better of the last iterate and the running average\n",
                P.max_iter, P.tol, late.c_str());
    if (tm) { tm->ms_loop = ms_loop; tm->ms_total = ms_since(t0); }
    return DESC_OK;
}

}  // namespace

extern "C" {

int desc_lp_batch_plan(const desc_problem* probs, int32_t count, const int32_t* nsample, int32_t* nsample_out, int64_t* m_pos, int64_t* var_off, int64_t* row_off,
                       int32_t* ncol, int32_t* nrow) {
    return no_throw("desc_lp_batch_plan", [&]() -> int {
        if (count < 0 || (count > 0 && !probs)) return fail(DESC_ERR_INVALID, "NULL argument or negative count");
        BatchCsr csr;
        LbPlan pl;
        const int rc = lb_plan(probs, count, nsample, &csr, pl);
        if (rc) return rc;
        if (nsample_out) std::copy(pl.nsample.begin(), pl.nsample.end(), nsample_out);
        if (m_pos) std::copy(pl.m_pos.begin(), pl.m_pos.end(), m_pos);
        if (var_off) std::copy(pl.var_off.begin(), pl.var_off.end(), var_off);
        if (row_off) std::copy(pl.row_off.begin(), pl.row_off.end(), row_off);
        if (ncol) std::copy(pl.ncol.begin(), pl.ncol.end(), ncol);
        if (nrow) std::copy(pl.nrow.begin(), pl.nrow.end(), nrow);
        return DESC_OK;
    });
}

int desc_lp_batch_create(const desc_problem* probs, int32_t count, const int32_t* nsample, const uint64_t* seeds, int32_t device, desc_lp_batch** out) {
    return batch_create_guarded("desc_lp_batch_create", out, probs, count, [&](desc_lp_batch* h) { return lb_create(probs, count, nsample, seeds, device, h); });
}

int desc_lp_batch_sizes(const desc_lp_batch* h, int32_t* count, int64_t* node_off, int64_t* edge_off, int32_t* nsample, int64_t* m_pos, int64_t* var_off, int64_t* row_off) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    const LbPlan& pl = h->plan;
    if (nsample) std::copy(pl.nsample.begin(), pl.nsample.end(), nsample);
    if (m_pos) std::copy(pl.m_pos.begin(), pl.m_pos.end(), m_pos);
    if (var_off) std::copy(pl.var_off.begin(), pl.var_off.end(), var_off);
    if (row_off) std::copy(pl.row_off.begin(), pl.row_off.end(), row_off);
    return batch_sizes(*h, count, node_off, edge_off);
}

int desc_lp_batch_get_samples(desc_lp_batch* h, int32_t* pos_edges, int32_t* k) {
    return no_throw("desc_lp_batch_get_samples", [&]() -> int {
        if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
        const LbPlan& pl = h->plan;
        if (pos_edges) std::copy(pl.pos.begin(), pl.pos.end(), pos_edges);
        if (!k || pl.MC == 0) return DESC_OK;
        DESC_HIP(hipSetDevice(h->device));
        DESC_HIP(hipMemcpyAsync(k, h->a.kk, sizeof(int32_t) * (size_t)pl.MC, hipMemcpyDeviceToHost, h->stream));
        DESC_HIP(hipStreamSynchronize(h->stream));
        for (int64_t c = 0; c < pl.MC; ++c) k[c] += 1;                   // 1-based, as CoIndMat
        return DESC_OK;
    });
}

int desc_lp_batch_run(desc_lp_batch* h, const desc_lp_params* params, double* s_vec, double* y, desc_lp_info* infos, desc_lp_batch_timings* timings) {
    return no_throw("desc_lp_batch_run", [&]() -> int {
        if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
        return lb_run(h, params, s_vec, y, infos, timings);
    });
}

void desc_lp_batch_destroy(desc_lp_batch* h) { delete h; }

}  // extern "C"

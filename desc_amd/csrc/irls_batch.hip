// IRLS_GM / IRLS_L12 (Algorithms/IRLS_GM.m, IRLS_L12.m; irls.hip) for many small problems in two launches (desc_irls_batch_*): the last two
// rows of Demo/compare_algorithms.m for a whole Monte-Carlo batch.
//
// irls.hip drives one problem with a host loop: thousands of tiny launches and hundreds of blocking read-backs (one per backtracking
// trial, two per primal-dual step, a probe every 5 CG steps, one per L1 and IRLS step).  Here
//   launch A  k_irls_project_batch   IRLS_GM.m:82-93 over the concatenated edges of the batch; per problem the smallest failing caller
//                                    row (integer atomicMin) and a warning count, which the host reads as B pairs of integers
//   launch B  k_irls_batch           one workgroup of 256 threads per problem runs stages 4 and 5 of desc_irls_run_dev from the projected
//                                    blocks to R_l1 and R: the spanning-tree start, the L1 loop with pd_solve's primal-dual steps and their
//                                    Newton systems, Q = r2q(q2r(Q)), the reweighted loop
// with no host round trip inside either.
//
// State.  The per-node arrays live in dynamic LDS, 34 doubles per node in the L1 stage (Q; the primal-dual x, Atv, w1p, dg, dx, Atdv; the
// PCG's r z p q) and the 26 of laa_wg.h in the reweighted stage, over the same block; a problem addresses it with its own n.  The
// per-edge arrays (QQ, B, w and the sixteen m x 3 arrays of the primal-dual state) lie in global memory at the problem's edge offset.
// The graph part of the spanning-tree start is host work (create): the passes over the edges in the caller's row order give a
// sequence of (edge, direction), which one thread walks with irls_tree_step.  The problems themselves (records, CSR, endpoints,
// rotations) are those of the resident problem set (problem_batch.h) the handle is created on, the caller's or one made from the
// caller's problem list; signs, edge -> problem map and identity row orders come from it by launches (batch_kernels.h).
//
// Arithmetic and summation orders.  Every per-element expression and every scalar rule is the text of irls_math.h and laa_math.h,
// which irls.hip and laa.hip call too.  The sums keep the single path's orders:
//   * k_pd_resid and k_pd_accept run on PD_RG = 256 blocks with a grid stride: block beta's partial is block_reduce over the elements
//     256 beta + t + 65536 k (and, in k_pd_resid, the node 256 beta + t added to the same accumulator), and the host adds the partials
//     in block order from 0.0.  The workgroup does exactly that for beta = 0, 1, ... up to the last non-empty block (an empty block's
//     partial is +0.0).  k_pd_accept's block_reduce<6, 0> reduces its six values by six independent copies of one tree: two
//     block_reduce<3, 0> give the same bits, and the kernel holds one instantiation's LDS (6 KiB) instead of two (18 KiB).
//   * the maxima and minima (k_pd_absmax, k_pd_dir's step bounds, the L1 score) do not depend on the order: wg_extreme.
//   * a CSR row is summed by the 16 lanes of a DPP row (pd_gather_row16), the Newton systems go through wg_pcg<true, true> and the
//     reweighted stage through wg_laa_step (laa_wg.h).
// The result is desc_irls_run's bit for bit.
//
// Control flow follows the rules at the top of laa_wg.h: every thread takes every decision from the same LDS values with the same
// instructions, the integers that steer loops and barriers go through readfirstlane, every loop is bounded by max_iter_l1, pdmaxiter,
// the 32 backtracking trials, cg_max, a row length or m.  No spinning on memory, no floating-point atomic, nothing between workgroups.
// The info array is preset to "never finished" (status -1); a workgroup writes its record when it is done.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "batch_csr.h"
#include "batch_device.h"
#include "batch_kernels.h"
#include "irls_math.h"
#include "problem_batch.h"
#include "laa_wg.h"

// A weak reference: the library loads next to a HIP runtime that lacks the call (the stand-in runtime of the host sanitizer test, which
// no batched IRLS runs on), and create refuses there instead of the loader.
extern "C" hipError_t hipFuncGetAttributes(struct hipFuncAttributes* attr, const void* func) __attribute__((weak));

namespace desc {
namespace {

constexpr int IB_NODE_DOUBLES = 4 + 10 * 3;            // Q; pd x, Atv, w1p, dg, dx, Atdv; the PCG's r z p q
constexpr int IB_STATIC_BYTES = 12 * 1024;             // set aside for the kernel's fixed LDS: block_reduce<3, 0>'s tree (6 KiB), scalars; checked at create
constexpr int IRLS_BATCH_MAX_N = (RB_LDS_BYTES - IB_STATIC_BYTES) / (8 * IB_NODE_DOUBLES);      // 557
static_assert(IB_NODE_DOUBLES >= RB_NODE_DOUBLES, "the reweighted stage runs in the L1 stage's block");
static_assert(IRLS_BATCH_MAX_N >= 278, "whatever the other batched rotation calls accept is accepted here");
constexpr int IB_EDGE_ARRAYS = 16;                     // Ax u f1 f2 l1 l2 w2 s1 s2 sx ev1 ev2 Adx du d1 d2, m x 3 each (y is B itself)

inline size_t ib_lds_bytes(int n) { return sizeof(double) * (size_t)IB_NODE_DOUBLES * (size_t)n; }

// status: 0 done, -1 the workgroup never finished
struct IbInfo {
    int32_t status, l1_iters, irls_iters, pd_steps, pd_ill, pd_stuck, pd_solves, cg_l1, cg_irls, cg_unconverged;
    double l1_score, irls_score, worst_sq;
};

struct IbArgs {
    const PbProb* prob;
    const int32_t* rowptr;      // problem b's n_b + 1 row starts at node_off[b] + b, counted inside the problem
    const int32_t* adj;         // 2 m_b local neighbour ids at 2 edge_off[b]
    const int32_t* adj_eid;     // 2 m_b local edge ids
    const int8_t* sgn;          // 2 m_b incidence signs (Build_Amatrix.m:10)
    const int32_t *ii, *jj;     // m_b local endpoints at edge_off[b]
    const int32_t* seq;         // n_b - 1 entries 2 e + dir of the spanning-tree start at node_off[b] - b
    const double* P;            // the projected blocks, 9 m_b at 9 edge_off[b] (launch A)
    Quat* QQ;                   // m_b
    double *B, *w;              // 3 m_b, m_b
    double* edge;               // IB_EDGE_ARRAYS arrays of 3 M doubles behind one another
    int64_t M;
    double *R_l1, *R_out;       // 9 n_b at 9 node_off[b]
    IbInfo* info;
    int32_t mode, max_l1, max_irls;
    double sigma;               // radians
};

// ---- launch A: IRLS_GM.m:82-93 over the edges of all problems (k_irls_project of irls.hip with per-problem flags) ----------------------
// flags[2 b] the smallest failing caller row of problem b (INT_MAX: none), flags[2 b + 1] its warnings.  only >= 0: that edge alone, its
// status / det / s into info[5].
__global__ __launch_bounds__(256) void k_irls_project_batch(const double* rij, const int32_t* order, const int32_t* eprob, int64_t M, double* P,
                                                            int32_t* flags, int64_t only, double* info) {
    const int64_t lo = only >= 0 ? only : 0, hi = only >= 0 ? only + 1 : M;
    for (int64_t e = lo + (int64_t)blockIdx.x * 256 + threadIdx.x; e < hi; e += (int64_t)gridDim.x * 256) {
        double a[9], v[9], s[3], det;
        const int status = irls_edge_status(rij + 9 * e, a, v, s, &det);
        if (only >= 0) {
            info[0] = status; info[1] = det; info[2] = s[0]; info[3] = s[1]; info[4] = s[2];
            continue;
        }
        const int b = eprob[e];
        if (status >= 2) atomicMin(flags + 2 * b, order[e]);
        else if (status == 1) atomicAdd(flags + 2 * b + 1, 1);
        irls_edge_project(a, v, s, P + 9 * e);
    }
}

// ---- launch B ---------------------------------------------------------------------------------------------------------------------------
// A maximum (OP 2) or minimum (OP 1) of K values per thread over the workgroup, into every thread's v[]: the waves by shuffles, the four
// waves through sh[4 K].  fmin / fmax skip NaN and the extreme of a set does not depend on the order it is taken in.  Holds two
// barriers: sh is free again when it returns.
template <int K, int OP>
__device__ __forceinline__ void wg_extreme(double (&v)[K], double* sh) {
    for (int k = 0; k < K; ++k)
        for (int off = 32; off >= 1; off >>= 1) { const double o = __shfl_xor(v[k], off); v[k] = OP == 1 ? fmin(v[k], o) : fmax(v[k], o); }
    if ((threadIdx.x & 63) == 0) for (int k = 0; k < K; ++k) sh[(threadIdx.x >> 6) * K + k] = v[k];
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        const double a = sh[k], b = sh[K + k], c = sh[2 * K + k], d = sh[3 * K + k];
        v[k] = OP == 1 ? fmin(fmin(a, b), fmin(c, d)) : fmax(fmax(a, b), fmax(c, d));
    }
    __syncthreads();
}

// the primal-dual state of one problem as its workgroup sees it (PdState of irls.hip)
struct WgPd {
    int n, m, nvb;                                      // nvb: the non-empty virtual blocks of the partial-reduction kernels
    const int32_t *rowptr, *adj, *eid, *ii, *jj;
    const int8_t* sgn;
    const double* y;                                    // B
    double *Ax, *u, *f1, *f2, *l1, *l2, *w2, *s1, *s2, *sx, *ev1, *ev2, *Adx, *du, *d1, *d2;     // m x 3, global
    double *x, *Atv, *w1p, *dg, *dx, *Atdv, *r, *z, *p, *q;                                      // n x 3, LDS
    double *part3, *sh;                                 // LDS: block_reduce's out[3]; wg_extreme's 24 doubles
};
struct PdCount { int steps = 0, ill = 0, stuck = 0, solves = 0; WgCg cg; };

// k_pd_gather<MODE> over the rows of the problem: out (n x 3, LDS).  Expects a barrier behind the last write of ev1 / ev2; ends with one.
template <int MODE>
__device__ __forceinline__ void wg_pd_gather(const WgPd& S, const double* ev1, const double* ev2, const double coef[3], double* out) {
    const int l16 = threadIdx.x & 15, row = threadIdx.x >> 4;
    for (int vb = 0; vb < S.n; vb += 16) {
        const int v = vb + row;
        const bool on = v < S.n && v > 0;
        double g[3], h[3];
        pd_gather_row16<MODE>(S.eid, S.sgn, ev1, ev2, on ? S.rowptr[v] : 0, on ? S.rowptr[v + 1] : 0, l16, g, h);
        if (v < S.n && l16 == 0)
            for (int c = 0; c < 3; ++c) out[3 * v + c] = pd_gather_out<MODE>(coef[c], g[c], h[c]);
    }
    __syncthreads();
}
// one virtual block's partial through block_reduce<3, 0>, added to tot as the host adds the partials: in block order
__device__ __forceinline__ void wg_add_partial(double (&acc)[3], double* tot, double* part3) {
    block_reduce<3, 0>(acc, part3);
    __syncthreads();
    for (int c = 0; c < 3; ++c) tot[c] = tot[c] + part3[c];
}
// k_pd_resid<TRIAL> on its 256 virtual blocks and read_part's sum: rr[3].  Expects a barrier behind the last write of what it reads.
template <bool TRIAL>
__device__ __forceinline__ void wg_pd_resid(const WgPd& S, const Pd3& a, double rr[3]) {
    const int tid = threadIdx.x;
    rr[0] = rr[1] = rr[2] = 0.0;
    for (int beta = 0; beta < S.nvb; ++beta) {
        double acc[3] = {0, 0, 0};
        for (int64_t e = (int64_t)beta * 256 + tid; e < S.m; e += (int64_t)PD_RG * 256)
            for (int c = 0; c < 3; ++c) {
                if (!a.act[c]) continue;
                acc[c] += pd_resid_edge<TRIAL>(a, c, 3 * e + c, S.y, S.Ax, S.u, S.l1, S.l2, S.Adx, S.du, S.d1, S.d2);
            }
        const int v = beta * 256 + tid;
        if (v < S.n && v != 0)
            for (int c = 0; c < 3; ++c) {
                if (!a.act[c]) continue;
                acc[c] += pd_resid_node<TRIAL>(a, c, v, S.Atv, S.Atdv);
            }
        wg_add_partial(acc, rr, S.part3);
    }
}
// k_pd_accept on its 256 virtual blocks and read_part's sum: dots[6].  Ends with a barrier behind its writes.
__device__ __forceinline__ void wg_pd_accept(const WgPd& S, const Pd3& a, double dots[6]) {
    const int tid = threadIdx.x;
    for (int k = 0; k < 6; ++k) dots[k] = 0.0;
    for (int beta = 0; beta < S.nvb; ++beta) {
        double acc1[3] = {0, 0, 0}, acc2[3] = {0, 0, 0};
        for (int64_t e = (int64_t)beta * 256 + tid; e < S.m; e += (int64_t)PD_RG * 256)
            for (int c = 0; c < 3; ++c) {
                const int64_t k = 3 * e + c;
                if (a.act[c]) pd_accept_at(a, c, k, S.y, S.Ax, S.u, S.l1, S.l2, S.f1, S.f2, S.Adx, S.du, S.d1, S.d2);
                acc1[c] += S.f1[k] * S.l1[k]; acc2[c] += S.f2[k] * S.l2[k];
            }
        const int v = beta * 256 + tid;
        if (v < S.n)
            for (int c = 0; c < 3; ++c)
                if (a.act[c]) pd_accept_node(a, c, v, S.x, S.Atv, S.dx, S.Atdv);
        wg_add_partial(acc1, dots, S.part3);
        wg_add_partial(acc2, dots + 3, S.part3);
    }
    __syncthreads();
}

// pd_solve of irls.hip: W(2:end, 2:4) = [l1decode_pd(0, A, [], B(:,c), eps, pdmaxiter, AtA) for c = 1..3] (BoxMedianSO3Graph.m:166-168)
// into S.x.  Expects a barrier behind the last write of B; ends with one.
__device__ __forceinline__ void wg_pd_solve(const WgPd& S, int pdmaxiter, int cg_max, PdCount& C) {
    const int tid = threadIdx.x, n = S.n, m = S.m;
    const double M = (double)m;
    for (int t = tid; t < 3 * n; t += 256) S.x[t] = 0.0;
    Pd3 a{}; for (int c = 0; c < 3; ++c) a.act[c] = 1;
    // ---- start (:268-287)
    {
        double v[3] = {0, 0, 0};
        for (int e = tid; e < m; e += 256)
            for (int c = 0; c < 3; ++c) v[c] = fmax(v[c], fabs(S.y[3 * (int64_t)e + c]));
        wg_extreme<3, 2>(v, S.sh);
        for (int c = 0; c < 3; ++c) a.ymax[c] = v[c];
    }
    for (int e = tid; e < m; e += 256)
        for (int c = 0; c < 3; ++c) pd_init_at(S.y, a.ymax[c], 3 * (int64_t)e + c, S.Ax, S.u, S.f1, S.f2, S.l1, S.l2, S.ev1);
    __syncthreads();
    wg_pd_gather<0>(S, S.ev1, nullptr, a.tau, S.Atv);
    double tau[3] = {0, 0, 0}, resnorm[3] = {0, 0, 0}, sdg[3] = {0, 0, 0}, dots[6];
    // sdg, tau, resnorm of the current point (:280-283, :347-350) for the coordinates in act, from the dots wg_pd_accept has just formed
    auto scalars = [&](const int act[3]) {
        Pd3 b{};
        for (int c = 0; c < 3; ++c) {
            if (!act[c]) continue;
            sdg[c] = pd_sdg(dots[c], dots[3 + c]);
            tau[c] = pd_tau(M, sdg[c]);
            b.act[c] = 1; b.tau[c] = tau[c];
        }
        double rr[3];
        wg_pd_resid<false>(S, b, rr);
        for (int c = 0; c < 3; ++c) if (act[c]) resnorm[c] = pd_resnorm(rr[c]);
    };
    int run[3] = {1, 1, 1};
    {
        const Pd3 none{};                                                // no coordinate moves: only the dots of the start
        wg_pd_accept(S, none, dots);
    }
    scalars(run);
    int pditer = 0;
    for (int c = 0; c < 3; ++c) run[c] = uni(pd_goes_on(sdg[c], pditer, pdmaxiter));           // :287
    while (uni((run[0] | run[1] | run[2]) && pditer < pdmaxiter)) {
        ++pditer;
        for (int c = 0; c < 3; ++c) { a.act[c] = run[c]; a.tau[c] = tau[c]; }
        // ---- Newton system (:296-312)
        for (int e = tid; e < m; e += 256)
            for (int c = 0; c < 3; ++c) pd_pre_at(a, c, 3 * (int64_t)e + c, S.f1, S.f2, S.l1, S.l2, S.w2, S.s1, S.s2, S.sx, S.ev1, S.ev2);
        __syncthreads();
        double coef[3];
        for (int c = 0; c < 3; ++c) coef[c] = pd_gather_coef(run[c], tau[c]);                 // w1 = -1/tau * (A' ...)
        wg_pd_gather<1>(S, S.ev1, S.ev2, coef, S.w1p);
        wg_pd_gather<2>(S, S.sx, nullptr, coef, S.dg);                                        // pd_pcg: the Jacobi diagonal
        ++C.solves;
        int bad[3];
        wg_pcg<true, true>(n, S.rowptr, S.adj, S.eid, S.sx, S.w1p, S.dg, S.dx, S.r, S.z, S.p, S.q, run, PD_PROBE, cg_max, C.cg, bad);
        for (int c = 0; c < 3; ++c)
            if (uni(bad[c])) { ++C.ill; run[c] = 0; a.act[c] = 0; }                           // :308-312
        if (!uni(run[0] | run[1] | run[2])) break;
        for (int c = 0; c < 3; ++c) if (run[c]) ++C.steps;
        // ---- direction and step length (:315-330)
        double mn[6] = {INFINITY, INFINITY, INFINITY, INFINITY, INFINITY, INFINITY};
        for (int e = tid; e < m; e += 256) {
            const int i = S.ii[e], j = S.jj[e];
            for (int c = 0; c < 3; ++c) pd_dir_at(a, c, e, i, j, S.dx, S.f1, S.f2, S.l1, S.l2, S.w2, S.s1, S.s2, S.Adx, S.du, S.d1, S.d2, S.ev1, mn);
        }
        wg_extreme<6, 1>(mn, S.sh);                                                           // holds the barrier behind ev1
        wg_pd_gather<0>(S, S.ev1, nullptr, coef, S.Atdv);
        double s[3] = {0, 0, 0};
        for (int c = 0; c < 3; ++c)
            if (run[c]) s[c] = pd_step_length(mn[c], mn[3 + c]);
        // ---- backtracking (:332-346): one trial of every searching coordinate per pass
        int search[3], backiter[3] = {0, 0, 0}, accept[3] = {0, 0, 0};
        double s_acc[3] = {0, 0, 0};
        for (int c = 0; c < 3; ++c) search[c] = run[c];
        for (int trial = 0; trial <= PD_MAX_BACKITER && uni(search[0] | search[1] | search[2]); ++trial) {
            Pd3 t{};
            for (int c = 0; c < 3; ++c) { t.act[c] = search[c]; t.s[c] = s[c]; t.tau[c] = tau[c]; }
            double rr[3];
            wg_pd_resid<true>(S, t, rr);
            for (int c = 0; c < 3; ++c) {
                if (!search[c]) continue;
                double s_tried;
                const int verdict = uni(pd_trial(rr[c], resnorm[c], &s[c], &backiter[c], &s_tried));
                if (verdict == PD_TRIAL_STUCK) { ++C.stuck; search[c] = 0; run[c] = 0; }      // :339-343
                else if (verdict == PD_TRIAL_ACCEPT) { search[c] = 0; accept[c] = 1; s_acc[c] = s_tried; }
            }
        }
        // ---- next iterate (:348-356)
        Pd3 acc{};
        for (int c = 0; c < 3; ++c) { acc.act[c] = accept[c]; acc.s[c] = s_acc[c]; }
        wg_pd_accept(S, acc, dots);
        scalars(accept);
        for (int c = 0; c < 3; ++c)
            if (accept[c]) run[c] = uni(pd_goes_on(sdg[c], pditer, pdmaxiter));
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_irls_batch(IbArgs a) {
    extern __shared__ double ib_lds[];
    __shared__ double sh_ext[24];
    __shared__ double sh_part3[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    const PbProb pd = a.prob[b];
    const int n = uni(pd.n), m = uni(pd.m);
    const int32_t* ii = a.ii + pd.edge_off;
    const int32_t* jj = a.jj + pd.edge_off;
    Quat* QQ = a.QQ + pd.edge_off;
    double* B = a.B + 3 * pd.edge_off;
    double* w = a.w + pd.edge_off;
    Quat* Q = (Quat*)ib_lds;
    WgPd S;
    S.n = n; S.m = m;
    S.nvb = min(PD_RG, (max(n, m) + 255) / 256);
    S.rowptr = a.rowptr + pd.node_off + b;
    S.adj = a.adj + 2 * pd.edge_off;
    S.eid = a.adj_eid + 2 * pd.edge_off;
    S.sgn = a.sgn + 2 * pd.edge_off;
    S.ii = ii; S.jj = jj; S.y = B;
    {
        double* eb = a.edge + 3 * pd.edge_off;          // array k of the primal-dual state at 3 (k M + edge_off)
        const int64_t st = 3 * a.M;
        S.Ax = eb; S.u = eb + st; S.f1 = eb + 2 * st; S.f2 = eb + 3 * st; S.l1 = eb + 4 * st; S.l2 = eb + 5 * st; S.w2 = eb + 6 * st;
        S.s1 = eb + 7 * st; S.s2 = eb + 8 * st; S.sx = eb + 9 * st; S.ev1 = eb + 10 * st; S.ev2 = eb + 11 * st; S.Adx = eb + 12 * st;
        S.du = eb + 13 * st; S.d1 = eb + 14 * st; S.d2 = eb + 15 * st;
        static_assert(IB_EDGE_ARRAYS == 16, "the sixteen arrays above");
        double* nb = ib_lds + 4 * n;                    // behind Q: ten n x 3 arrays
        S.x = nb; S.Atv = nb + 3 * n; S.w1p = nb + 6 * n; S.dg = nb + 9 * n; S.dx = nb + 12 * n; S.Atdv = nb + 15 * n;
        S.r = nb + 18 * n; S.z = nb + 21 * n; S.p = nb + 24 * n; S.q = nb + 27 * n;
    }
    S.part3 = sh_part3; S.sh = sh_ext;
    const int cg_max = min(20000, 20 * n + 200);

    // ---- stage 4, the start: QQ of the projected blocks (laa_set_qq), the spanning-tree start (BoxMedianSO3Graph.m:78-114)
    {
        const double* P = a.P + 9 * pd.edge_off;
        for (int e = tid; e < m; e += 256) QQ[e] = r2q(P + 9 * (int64_t)e, false);
    }
    for (int v = tid; v < n; v += 256) Q[v] = Quat{1.0, 0.0, 0.0, 0.0};                         // :78
    __syncthreads();
    if (tid == 0) {
        const int32_t* seq = a.seq + pd.node_off - b;
        for (int t = 0; t < n - 1; ++t) { const int32_t en = seq[t]; irls_tree_step(en, QQ[en >> 1], ii, jj, Q); }
    }
    __syncthreads();
    // ---- the L1 loop (:134-187)
    PdCount C;
    double changeThreshold = .001, score = INFINITY;                                           // :56, :134
    int Iteration = 0, L1Step = 2;
    while (uni(l1_goes_on(score, changeThreshold, L1Step, Iteration, a.max_l1))) {             // :138
        l1_step_rule(score, &changeThreshold, &L1Step);                                        // :139
        L1Step = uni(L1Step);
        for (int e = tid; e < m; e += 256) edge_log(QQ[e], Q[ii[e]], Q[jj[e]], B + 3 * (int64_t)e);   // :141-160
        __syncthreads();
        wg_pd_solve(S, L1Step, cg_max, C);                                                     // :162-168
        double sc[1] = {0.0};
        for (int v = tid; v < n; v += 256) {                                                   // :173-185
            const double theta = l1_node_update(S.x + 3 * v, Q + v);
            if (v > 0) sc[0] = fmax(sc[0], theta);
        }
        wg_extreme<1, 2>(sc, sh_ext);
        score = sc[0];
        ++Iteration;
    }
    const int l1_iters = Iteration;
    const double l1_score = score;
    // ---- R_l1 = real(q2R(Q)) (:192-197); stage 5 starts from Q = R2Q(R_l1) (RobustMeanSO3Graph.m:75-80) and w = 1 (:127)
    for (int v = tid; v < n; v += 256) {
        double Mx[9];
        q2r(Q[v], Mx);
        double* o = a.R_l1 + 9 * (pd.node_off + v);
        for (int c = 0; c < 9; ++c) o[c] = Mx[c];
        Q[v] = r2q(Mx, false);
    }
    for (int e = tid; e < m; e += 256) w[e] = 1.0;
    WgLaa st;                                           // laa_wg.h: the problem's state and the step on it
    st.n = n; st.m = m;
    st.rowptr = S.rowptr; st.adj = S.adj; st.eid = S.eid; st.sgn = S.sgn;
    st.ii = ii; st.jj = jj; st.QQ = QQ; st.B = B; st.w = w;
    wg_laa_views(ib_lds, n, st);
    __syncthreads();
    WgCg cg;
    score = INFINITY;
    Iteration = 0;
    while (uni(irls_goes_on(score, Iteration, a.max_irls))) {                                  // :130
        score = wg_laa_step(st, cg_max, cg);                                                   // :132-186
        for (int e = tid; e < m; e += 256) w[e] = irls_weight(edge_residual_sq(st.x, B, ii, jj, e), a.mode, a.sigma);   // :169-171
        __syncthreads();
        ++Iteration;
    }
    for (int v = tid; v < n; v += 256) {                                                       // q2R (:193-197)
        double Mx[9];
        q2r(Q[v], Mx);
        double* o = a.R_out + 9 * (pd.node_off + v);
        for (int c = 0; c < 9; ++c) o[c] = Mx[c];
    }
    if (tid == 0) {
        IbInfo o;
        o.status = 0; o.l1_iters = l1_iters; o.irls_iters = Iteration; o.pd_steps = C.steps; o.pd_ill = C.ill; o.pd_stuck = C.stuck;
        o.pd_solves = C.solves; o.cg_l1 = C.cg.total; o.cg_irls = cg.total; o.cg_unconverged = C.cg.unconverged + cg.unconverged;
        o.l1_score = l1_score; o.irls_score = score; o.worst_sq = C.cg.worst_sq < cg.worst_sq ? cg.worst_sq : C.cg.worst_sq;
        a.info[b] = o;
    }
}

// identity orders: order[edge_off[b] + e] = e, the caller's row of every edge, without an upload
__global__ __launch_bounds__(256) void k_irls_identity_order(const PbProb* prob, int32_t* order) {
    const PbProb pd = prob[blockIdx.x];
    for (int e = threadIdx.x; e < pd.m; e += 256) order[pd.edge_off + e] = e;
}

}  // namespace
}  // namespace desc

using namespace desc;

struct desc_irls_batch : desc::BatchCsr, desc::BatchDevice {    // the set's offsets and endpoints; device, stream, arena, events
    hvec<int32_t> order;                                // the caller's row of every edge, inside its problem
    hvec<int32_t> seq;                                  // the spanning-tree start: problem b's n_b - 1 entries at node_off[b] - b
    hvec<int32_t> flags0;                               // launch A's flags before the launch: {INT_MAX, 0} per problem
    const PbProb* d_prob = nullptr;
    const int32_t *d_rowptr = nullptr, *d_adj = nullptr, *d_adj_eid = nullptr, *d_ii = nullptr, *d_jj = nullptr;
    int32_t *d_seq = nullptr, *d_order = nullptr, *d_eprob = nullptr, *d_flags = nullptr;
    int8_t* d_sgn = nullptr;
    const double* d_rij = nullptr;
    double *d_P = nullptr, *d_B = nullptr, *d_w = nullptr, *d_edge = nullptr, *d_Rl1 = nullptr, *d_Rout = nullptr, *d_einfo = nullptr;
    Quat* d_QQ = nullptr;
    IbInfo* d_info = nullptr;
    std::shared_ptr<desc::PbSet> set;         // the owner of d_prob, the CSR, d_ii / d_jj and d_rij
    bool own_set = false;                     // the handle made the set from a problem list and is its only owner
    ~desc_irls_batch() { close(); }           // the stream drains before the set may go
};

namespace {

// One problem's spanning-tree sequence from its edges and the caller's row of each (order nullable: the edge order itself); refuses an
// order that is no permutation.  *reached: the nodes the passes reach (n when the graph is connected).
int ib_tree(const desc_problem& q, const int32_t* order, hvec<int32_t>& visit, hvec<int32_t>& seq, int64_t* reached) {
    const int64_t m = q.m;
    visit.assign((size_t)m, -1);
    for (int64_t e = 0; e < m; ++e) {
        const int64_t r = order ? order[e] : e;
        if (r < 0 || r >= m || visit[(size_t)r] >= 0) return fail(DESC_ERR_INVALID, "order must be a permutation of 0..m-1");
        visit[(size_t)r] = (int32_t)e;
    }
    *reached = irls_tree_sequence(q.n, q.ind_i, q.ind_j, visit.data(), m, seq);
    return DESC_OK;
}

int ib_check_n(int32_t b, int64_t n) {
    if (n > IRLS_BATCH_MAX_N)
        return fail(DESC_ERR_INVALID, "problem %d: n = %lld exceeds %d (the per-node state of the L1 stage must fit the LDS of one workgroup): solve it with IRLS_GM / IRLS_L12",
                    b, (long long)n, IRLS_BATCH_MAX_N);
    return DESC_OK;
}

// The caller's row orders and the tree sequences of every problem into h->order / h->seq, h's offsets being set; probs[b] needs n, m and
// the endpoints alone.  Refuses an order that is no permutation and a graph that is not connected.
int ib_orders_and_trees(const desc_problem* probs, int32_t count, const int32_t* const* orders, desc_irls_batch* h) {
    h->order.resize((size_t)h->M);
    h->seq.assign((size_t)std::max<int64_t>(h->N - count, 1), 0);
    hvec<int32_t> visit, seq;
    int rc;
    for (int32_t b = 0; b < count; ++b) {
        const int32_t* od = orders ? orders[b] : nullptr;
        int64_t reached = 0;
        if ((rc = ib_tree(probs[b], od, visit, seq, &reached))) { const std::string msg = desc_last_error(); return fail(rc, "problem %d: %s", b, msg.c_str()); }
        if (reached < probs[b].n)
            return fail(DESC_ERR_INVALID, "problem %d: the graph is not connected (%lld of %lld nodes reached from node 1): solve it with IRLS_GM / IRLS_L12",
                        b, (long long)reached, (long long)probs[b].n);
        const int64_t eo = h->edge_off[(size_t)b];
        for (int64_t e = 0; e < probs[b].m; ++e) h->order[(size_t)(eo + e)] = od ? od[e] : (int32_t)e;
        std::copy(seq.begin(), seq.end(), h->seq.begin() + (h->node_off[(size_t)b] - b));
    }
    return DESC_OK;
}

void ib_flags0(desc_irls_batch* h) {
    h->flags0.resize(2 * (size_t)h->count);
    for (int32_t b = 0; b < h->count; ++b) { h->flags0[2 * (size_t)b] = INT_MAX; h->flags0[2 * (size_t)b + 1] = 0; }
}

// the kernel's fixed LDS against what was set aside for it: an error at create instead of a failed launch
int ib_check_lds(const desc_irls_batch* h) {
    hipFuncAttributes fa;
    if (!&hipFuncGetAttributes) return fail(DESC_ERR_HIP, "the HIP runtime exports no hipFuncGetAttributes: the LDS budget of the batched IRLS cannot be checked");
    DESC_HIP(hipFuncGetAttributes(&fa, (const void*)k_irls_batch));
    if (fa.sharedSizeBytes > (size_t)IB_STATIC_BYTES || fa.sharedSizeBytes + ib_lds_bytes(h->max_n) > (size_t)RB_LDS_BYTES)
        return fail(DESC_ERR_STATE, "LDS budget exceeded: %zu bytes fixed, %zu bytes for n = %d, %d allowed", (size_t)fa.sharedSizeBytes,
                    ib_lds_bytes(h->max_n), (int)h->max_n, RB_LDS_BYTES);
    return DESC_OK;
}

// the run's own buffers; drains the stream
int ib_alloc_work(desc_irls_batch* h) {
    const size_t M = (size_t)h->M, N = (size_t)h->N, count = (size_t)h->count;
    int rc;
    if ((rc = h->mem.alloc(&h->d_P, 9 * M)) || (rc = h->mem.alloc(&h->d_QQ, M)) || (rc = h->mem.alloc(&h->d_B, 3 * M)) ||
        (rc = h->mem.alloc(&h->d_w, M)) || (rc = h->mem.alloc(&h->d_edge, (size_t)IB_EDGE_ARRAYS * 3 * M)) || (rc = h->mem.alloc(&h->d_Rl1, 9 * N)) ||
        (rc = h->mem.alloc(&h->d_Rout, 9 * N)) || (rc = h->mem.alloc(&h->d_info, count)) || (rc = h->mem.alloc(&h->d_flags, 2 * count)) ||
        (rc = h->mem.alloc(&h->d_einfo, 5)))
        return rc;
    // the largest dynamic LDS any handle may ask for: the attribute belongs to the kernel, not to a handle, so it is never lowered
    DESC_HIP(hipFuncSetAttribute((const void*)k_irls_batch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ib_lds_bytes(IRLS_BATCH_MAX_N)));
    DESC_HIP(hipStreamSynchronize(h->stream));         // the caller's staging vectors may go
    return DESC_OK;
}

// The one create body, on a resident set: the caller's (desc_irls_batch_create_on, probs = NULL), or one the handle makes from probs and
// owns alone (the list path; the cap is then refused per problem inside the set's host part, between the other refusals of that
// problem).  The row orders and the tree sequences come from slices of the set's host endpoints (no rotation and no CSR is read).
// Uploads: the tree sequences, and the row orders only where one is not the identity; the problem records, the CSR, the endpoints and
// the rotations are the set's; the signs, the edge -> problem map and identity orders are formed by launches.
int ib_create(const desc_problem* probs, int32_t count, int32_t device, std::shared_ptr<PbSet> set, const int32_t* const* orders, desc_irls_batch* h) {
    auto t0 = std::chrono::steady_clock::now();
    int rc;
    h->own_set = !set;
    if (h->own_set) {
        set = std::make_shared<PbSet>();
        if ((rc = pb_host_part(probs, count, DESC_BUILD_HOST, [](int32_t b, const desc_problem& q) -> int { return ib_check_n(b, q.n); }, set.get()))) return rc;
    } else {
        for (int32_t b = 0; b < set->count; ++b)
            if ((rc = ib_check_n(b, set->node_off[(size_t)b + 1] - set->node_off[(size_t)b]))) return rc;
    }
    count = set->count;
    h->set = set;
    pb_share_host(*set, h, !h->own_set);             // an own set: h->ii / h->jj stay EMPTY until pb_take_endpoints below -- read set->ii / set->jj till then
    hvec<desc_problem> view((size_t)count);
    for (int32_t b = 0; b < count; ++b) {
        const size_t eo = (size_t)h->edge_off[(size_t)b];
        view[(size_t)b] = desc_problem{h->node_off[(size_t)b + 1] - h->node_off[(size_t)b], h->edge_off[(size_t)b + 1] - h->edge_off[(size_t)b],
                                       set->ii.data() + eo, set->jj.data() + eo, nullptr};
    }
    if ((rc = ib_orders_and_trees(view.data(), count, orders, h))) return rc;
    bool identity = true;
    for (int64_t b = 0; b < count && identity; ++b)
        for (int64_t e = h->edge_off[(size_t)b]; e < h->edge_off[(size_t)b + 1] && identity; ++e) identity = h->order[(size_t)e] == (int32_t)(e - h->edge_off[(size_t)b]);
    ib_flags0(h);
    h->ms_structure = ms_since(t0);
    if (count == 0) return DESC_OK;

    const char* what = "the batched IRLS";
    if (h->own_set) {                                  // nothing above touched the device
        if ((rc = pb_device_part(probs, device, what, set.get()))) return rc;
        pb_take_endpoints(*set, h);
    }
    if ((rc = h->open(set->device, what))) return rc;
    auto t1 = std::chrono::steady_clock::now();
    if ((rc = ib_check_lds(h))) return rc;
    h->d_prob = set->d_prob; h->d_rowptr = set->d_rowptr; h->d_adj = set->d_adj; h->d_adj_eid = set->d_adj_eid; h->d_ii = set->d_ii; h->d_jj = set->d_jj;
    h->d_rij = set->d_rij;
    const size_t M = (size_t)h->M;
    const dim3 grid((unsigned)count), block(256);
    if ((rc = h->upload(&h->d_seq, h->seq.data(), h->seq.size())) || (rc = h->mem.alloc(&h->d_sgn, 2 * M)) || (rc = h->mem.alloc(&h->d_eprob, M))) return rc;
    if (identity) {
        if ((rc = h->mem.alloc(&h->d_order, M))) return rc;
        hipLaunchKernelGGL(k_irls_identity_order, grid, block, 0, h->stream, h->d_prob, h->d_order);
    } else if ((rc = h->upload(&h->d_order, h->order.data(), M))) return rc;
    hipLaunchKernelGGL(k_batch_sgn<PbProb>, grid, block, 0, h->stream, h->d_prob, h->d_rowptr, h->d_adj, h->d_sgn);
    hipLaunchKernelGGL(k_batch_eprob<PbProb>, grid, block, 0, h->stream, h->d_prob, h->d_eprob);
    DESC_HIP(hipGetLastError());
    if ((rc = ib_alloc_work(h))) return rc;
    h->ms_upload = ms_since(t1) + (h->own_set ? set->ms_upload : 0);
    return DESC_OK;
}

int ib_run(desc_irls_batch* h, int32_t mode, double sigma_deg, int32_t max_iter_l1, int32_t max_iter_irls, double* R_out, double* R_l1,
           desc_irls_info* infos, desc_irls_batch_timings* tm) {
    auto t0 = std::chrono::steady_clock::now();
    const int32_t count = h->count;
    if (tm) { tm->ms_structure = h->ms_structure; tm->ms_upload = h->ms_upload; tm->ms_project = 0; tm->ms_solve = 0; tm->ms_total = 0; }
    if (mode != DESC_IRLS_GM && mode != DESC_IRLS_L12) return fail(DESC_ERR_INVALID, "mode must be DESC_IRLS_GM or DESC_IRLS_L12");
    if (count == 0) { if (tm) tm->ms_total = ms_since(t0); return DESC_OK; }
    if (!R_out || !infos) return fail(DESC_ERR_INVALID, "R_out or infos is NULL");
    const int max_l1 = max_iter_l1 > 0 ? max_iter_l1 : 10, max_irls = max_iter_irls > 0 ? max_iter_irls : 100;
    const double sigma = (sigma_deg > 0 ? sigma_deg : 5.0) * M_PI / 180.0;                     // RobustMeanSO3Graph.m:60
    int rc;
    DESC_HIP(hipSetDevice(h->device));
    const size_t M = (size_t)h->M, N = (size_t)h->N;
    // ---- launch A: checks and projection of every edge (IRLS_GM.m:82-93)
    DESC_HIP(hipMemcpyAsync(h->d_flags, h->flags0.data(), sizeof(int32_t) * 2 * (size_t)count, hipMemcpyHostToDevice, h->stream));
    DESC_HIP(hipMemsetAsync(h->d_info, 0xFF, sizeof(IbInfo) * (size_t)count, h->stream));      // status -1: the workgroup never finished
    hipLaunchKernelGGL(k_irls_project_batch, dim3(grid_for((int64_t)M, 2048)), dim3(256), 0, h->stream, h->d_rij, h->d_order, h->d_eprob, (int64_t)M,
                       h->d_P, h->d_flags, (int64_t)-1, h->d_einfo);
    DESC_HIP(hipGetLastError());
    hvec<int32_t> flags(2 * (size_t)count);
    DESC_HIP(hipMemcpyAsync(flags.data(), h->d_flags, sizeof(int32_t) * 2 * (size_t)count, hipMemcpyDeviceToHost, h->stream));
    DESC_HIP(hipStreamSynchronize(h->stream));
    for (int32_t b = 0; b < count; ++b) {
        const int32_t row = flags[2 * (size_t)b];
        if (row == INT_MAX) continue;
        const int64_t eo = h->edge_off[(size_t)b];
        int64_t e = eo;
        for (int64_t t = eo; t < h->edge_off[(size_t)b + 1]; ++t) if (h->order[(size_t)t] == row) { e = t; break; }
        hipLaunchKernelGGL(k_irls_project_batch, dim3(1), dim3(256), 0, h->stream, h->d_rij, h->d_order, h->d_eprob, (int64_t)M, h->d_P, h->d_flags, e,
                           h->d_einfo);
        DESC_HIP(hipGetLastError());
        double ei[5];
        DESC_HIP(hipMemcpyAsync(ei, h->d_einfo, sizeof ei, hipMemcpyDeviceToHost, h->stream));
        DESC_HIP(hipStreamSynchronize(h->stream));
        if (ei[0] == 3) return fail(DESC_ERR_INVALID, "problem %d: det(RR(:,:,%d))=%f", b, (int)row + 1, ei[1]);
        return fail(DESC_ERR_INVALID, "problem %d: svd(RR(:,:,%d))=[%f %f %f]", b, (int)row + 1, ei[2], ei[3], ei[4]);
    }
    const double ms_project = ms_since(t0);
    // ---- launch B: stages 4 and 5 of every problem
    IbArgs a{};
    a.prob = h->d_prob; a.rowptr = h->d_rowptr; a.adj = h->d_adj; a.adj_eid = h->d_adj_eid; a.sgn = h->d_sgn; a.ii = h->d_ii; a.jj = h->d_jj;
    a.seq = h->d_seq; a.P = h->d_P; a.QQ = h->d_QQ; a.B = h->d_B; a.w = h->d_w; a.edge = h->d_edge; a.M = (int64_t)M; a.R_l1 = h->d_Rl1;
    a.R_out = h->d_Rout; a.info = h->d_info; a.mode = mode; a.max_l1 = max_l1; a.max_irls = max_irls; a.sigma = sigma;
    const size_t lds = ib_lds_bytes(h->max_n);
    if (lds + IB_STATIC_BYTES > (size_t)RB_LDS_BYTES) return fail(DESC_ERR_STATE, "LDS budget exceeded (%zu bytes)", lds);
    if ((rc = h->timer_begin())) return rc;
    hipLaunchKernelGGL(k_irls_batch, dim3((unsigned)count), dim3(256), lds, h->stream, a);
    DESC_HIP(hipGetLastError());
    if ((rc = h->timer_end())) return rc;
    hvec<IbInfo> inf((size_t)count);
    hvec<double> R(9 * N), R1(9 * N);
    DESC_HIP(hipMemcpyAsync(inf.data(), h->d_info, sizeof(IbInfo) * (size_t)count, hipMemcpyDeviceToHost, h->stream));
    DESC_HIP(hipMemcpyAsync(R.data(), h->d_Rout, sizeof(double) * 9 * N, hipMemcpyDeviceToHost, h->stream));
    DESC_HIP(hipMemcpyAsync(R1.data(), h->d_Rl1, sizeof(double) * 9 * N, hipMemcpyDeviceToHost, h->stream));
    DESC_HIP(hipStreamSynchronize(h->stream));
    float ms = 0;
    if ((rc = h->timer_ms(&ms))) return rc;
    for (int32_t b = 0; b < count; ++b)
        if (inf[(size_t)b].status) return fail(DESC_ERR_STATE, "problem %d: the IRLS kernel did not finish (status %d)", b, (int)inf[(size_t)b].status);
    std::memcpy(R_out, R.data(), sizeof(double) * 9 * N);
    if (R_l1) std::memcpy(R_l1, R1.data(), sizeof(double) * 9 * N);
    const double ms_total = ms_since(t0);
    for (int32_t b = 0; b < count; ++b) {
        const IbInfo& g = inf[(size_t)b];
        desc_irls_info o{};
        o.comp_nodes = h->node_off[(size_t)b + 1] - h->node_off[(size_t)b]; o.comp_edges = h->edge_off[(size_t)b + 1] - h->edge_off[(size_t)b];
        o.l1_iters = g.l1_iters; o.irls_iters = g.irls_iters; o.l1_score = g.l1_score; o.irls_score = g.irls_score;
        o.pd_steps = g.pd_steps; o.pd_ill = g.pd_ill; o.pd_stuck = g.pd_stuck; o.pd_solves = g.pd_solves;
        o.warned_edges = flags[2 * (size_t)b + 1];
        o.cg_iters_l1 = g.cg_l1; o.cg_iters_irls = g.cg_irls; o.cg_unconverged = g.cg_unconverged;
        o.cg_residual = std::sqrt(g.worst_sq);          // sqrt is monotone: the largest |r|/|b| is the root of the largest ratio
        o.ms_total = ms_total;
        infos[b] = o;
    }
    if (tm) { tm->ms_project = ms_project; tm->ms_solve = ms; tm->ms_total = ms_total; }
    return DESC_OK;
}

}  // namespace

extern "C" {

int32_t desc_irls_batch_max_n(void) { return IRLS_BATCH_MAX_N; }

int desc_irls_batch_create(const desc_problem* probs, int32_t count, const int32_t* const* orders, int32_t device, desc_irls_batch** out) {
    return batch_create_guarded("desc_irls_batch_create", out, probs, count, [&](desc_irls_batch* h) { return ib_create(probs, count, device, nullptr, orders, h); });
}

int desc_irls_batch_create_on(desc_problem_batch* set, const int32_t* const* orders, desc_irls_batch** out) {
    return batch_create_guarded("desc_irls_batch_create_on", out, set, 0, [&](desc_irls_batch* h) { return ib_create(nullptr, 0, 0, set->s, orders, h); }, set != nullptr);
}

int desc_irls_batch_bytes(const desc_irls_batch* h, int64_t* h2d, int64_t* d2h) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    return batch_bytes_on_set(*h, h->own_set ? h->set.get() : nullptr, h2d, d2h);
}

int desc_irls_batch_sizes(const desc_irls_batch* h, int32_t* count, int64_t* node_off, int64_t* edge_off) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    return batch_sizes(*h, count, node_off, edge_off);
}

int desc_irls_batch_run(desc_irls_batch* h, int32_t mode, double sigma_deg, int32_t max_iter_l1, int32_t max_iter_irls, double* R_out, double* R_l1,
                        desc_irls_info* infos, desc_irls_batch_timings* timings) {
    return no_throw("desc_irls_batch_run", [&]() -> int {
        if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
        return ib_run(h, mode, sigma_deg, max_iter_l1, max_iter_irls, R_out, R_l1, infos, timings);
    });
}

void desc_irls_batch_destroy(desc_irls_batch* h) { delete h; }

int desc_irls_tree_sequence(const desc_problem* prob, const int32_t* order, int32_t* seq, int64_t* reached) {
    return no_throw("desc_irls_tree_sequence", [&]() -> int {
        if (!prob || !reached) return fail(DESC_ERR_INVALID, "NULL argument");
        int rc = validate_problem(prob, false);
        if (rc) return rc;
        if (prob->m == 0) return fail(DESC_ERR_INVALID, "empty edge list");
        hvec<int32_t> visit, s;
        if ((rc = ib_tree(*prob, order, visit, s, reached))) return rc;
        if (seq) std::copy(s.begin(), s.end(), seq);
        return DESC_OK;
    });
}

}  // extern "C"

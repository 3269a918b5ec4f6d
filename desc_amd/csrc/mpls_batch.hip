// The MPLS loop (Algorithms/MPLS.m:196-254) for many small problems in one launch (desc_mpls_batch_run): the last stage of the "MPLS"
// row of Demo/compare_algorithms.m for a whole Monte-Carlo batch, behind desc_cemp_batch_* (CEMP) and desc_mst_batch_run (the tree).
//
// mpls.hip runs one problem per call with a host-driven loop: per iteration laa_step's seven launches per PCG step and its blocking
// probe every 25 steps, the residual launch, the H-step launch, two or three read-backs for the quantile and a weights launch, up to 99
// times over.  Here ONE launch runs the loop of desc_mpls_run_dev for all B problems: one workgroup of 256 threads per problem, from
// Q = R2Q(R_init) to q2R, without a host round trip.
//
// State.  The loop runs on a CEMP batch handle (cemp_batch.h), which owns the CSR, the rotations and the sampled cycles (e_jk, e_ki, S0,
// has_cycle: nsample slots per edge of the batch, batch-global edge ids).  The per-node arrays live in LDS, 26 doubles per node, as in
// k_refine_batch (laa_wg.h); the LDS of a launch is sized from the largest problem of the batch and a problem addresses it with its own
// n.  The per-edge arrays QQ, B, w, Res, RH lie in global memory at the problem's edge offset; the handle allocates them and forms the
// incidence signs by a launch at its first loop.
//
// Arithmetic and summation orders.  The Weighted-LAA step and the quantile are the text k_refine_batch runs (laa_wg.h), which
// reproduces the single path's reductions; the residual is k_mpls_res's expression; the H step of an edge with cycles is
// cemp_edge_round (cemp_math.h) by one wave -- sample s on lane s & 63, sums by group_sum<64> -- with cemp_store<true>'s epilogue, that
// of an edge without cycles k_mpls_res's loop of nsample additions.  An edge belongs to exactly one wave, so the distribution of the
// edges over the four waves enters no result.  beta, tau and alpha of iteration it come from three device tables the host pads by
// repeating the last entry (padded() of mpls.hip).  The result is desc_mpls_run's loop bit for bit.
//
// Control flow.  As k_refine_batch: every decision around a barrier is taken by every thread from the same LDS values and goes through
// readfirstlane; every loop is bounded by max_iter, cg_max, a row length, m, nsample or the 8 digit passes.  There is no grid-wide
// barrier, no spinning on memory, nothing between workgroups and no floating-point atomic.  A problem whose selection finds no
// candidate or whose score is not finite writes its status word and leaves; the status words are preset to -1, so a workgroup that
// never finished is detected.
//
// Composition independence.  Problem b's workgroup reads b's arrays and b's sample slots and writes b's ranges; thread roles, loop
// bounds and summation orders are functions of b's n, m, CSR and nsample alone.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "batch_kernels.h"
#include "cemp_batch.h"
#include "cemp_math.h"
#include "laa_wg.h"

namespace desc {
namespace {

struct MbArgs {
    const CbProb* prob;
    const int32_t *rowptr, *adj, *adj_eid;      // the handle's per-problem CSR (local ids)
    const int8_t* sgn;                          // 2 m_b incidence signs (Build_Amatrix.m:10): -1 where the row's node is the edge's smaller endpoint
    const int32_t *ii, *jj;
    const double* rij;
    const int32_t *e_jk, *e_ki;                 // M * nsample batch-global edge ids
    const double* S0;                           // M * nsample
    const uint8_t* has_cycle;                   // M
    const double* S;                            // CEMP's SVec, M
    const double* R_init;                       // 9 n_b at 9 node_off[b]
    double* R_out;
    Quat* QQ;                                   // M
    double *B, *w, *Res, *RH;                   // 3 M, M, M, M
    MbInfo* info;
    const double *beta, *tau, *alpha;           // max(1, max_iter - 1) entries each: iteration it reads entry it - 1
    double stop_threshold;
    int32_t max_iter, nsample;
};

__global__ __launch_bounds__(256) void k_mpls_batch(MbArgs a) {
    extern __shared__ double mb_lds[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = uni(tid >> 6);
    const CbProb pd = a.prob[b];
    const int n = uni(pd.n), m = uni(pd.m), eo = uni(pd.edge_off), no = uni(pd.node_off);
    const int nsample = a.nsample;
    const int32_t* ii = a.ii + eo;
    const int32_t* jj = a.jj + eo;
    const double* S = a.S + eo;
    Quat* QQ = a.QQ + eo;
    double* B = a.B + 3 * (int64_t)eo;
    double* w = a.w + eo;
    double* Res = a.Res + eo;
    double* RH = a.RH + eo;
    WgLaa st;                                           // laa_wg.h: the problem's state and the step on it
    st.n = n; st.m = m;
    st.rowptr = a.rowptr + no + b;
    st.adj = a.adj + 2 * (int64_t)eo;
    st.eid = a.adj_eid + 2 * (int64_t)eo;
    st.sgn = a.sgn + 2 * (int64_t)eo;
    st.ii = ii; st.jj = jj; st.QQ = QQ; st.B = B; st.w = w;
    wg_laa_views(mb_lds, n, st);
    Quat* Q = st.Q;
    const double* Wv = st.Wv;

    // ---- laa_setup: Q = R2Q(R_init), QQ = R2Q(permute(RijMat, [2,1,3])); the initial weights, clipped and not truncated (MPLS.m:200-213)
    for (int v = tid; v < n; v += 256) Q[v] = r2q(a.R_init + 9 * ((int64_t)no + v), false);
    {
        const double* rij = a.rij + 9 * (int64_t)eo;
        for (int e = tid; e < m; e += 256) { QQ[e] = r2q(rij + 9 * (int64_t)e, true); w[e] = laa_weight(S[e], INFINITY, 1e4, 1e-4); }
    }
    __syncthreads();

    const double stop = a.stop_threshold;
    const int max_iter = a.max_iter;
    const int cg_max = min(20000, 20 * n + 200);
    double score = INFINITY;
    WgCg cg;
    int it = 1, status = 0;
    while (uni(score > stop && it < max_iter)) {                                            // MPLS.m:218
        const double beta = a.beta[it - 1], tau = a.tau[it - 1], alpha = a.alpha[it - 1];
        score = wg_laa_step(st, cg_max, cg);                                                // :220
        if (uni(!isfinite(score))) { status = 2; break; }
        // ---- :221-222, k_mpls_res
        for (int e = tid; e < m; e += 256) Res[e] = sqrt(edge_residual_sq(Wv, B, ii, jj, e)) / M_PI;
        __syncthreads();                                                                    // all of Res, before any wave gathers from it
        // ---- the H step (:223-240): one wave per edge
        for (int e = wv; e < m; e += 4) {
            const int g = eo + e;                                                           // the sample arrays hold batch-global edge ids
            if (uni(a.has_cycle[g])) {
                const double acc = cemp_edge_round((int64_t)g, lane, nsample, beta, a.e_jk, a.e_ki, a.S0, a.Res);      // cemp_math.h
                if (lane == 0) RH[e] = (1.0 - alpha) * Res[e] + alpha * acc;                // cemp_store<true>
            } else if (lane == 0) {
                const double r = Res[e];
                const double s0 = fabs(acos((0.0 - 1.0) / 2.0)) / M_PI, wq = 1.0 / (double)nsample;      // :130 on a zero cycle matrix
                double h = 0.0;
                for (int t = 0; t < nsample; ++t) h += wq * s0;                             // :236-237
                RH[e] = (1.0 - alpha) * r + alpha * h;
            }
        }
        __syncthreads();                                                                    // all of RH
        // ---- :241-245: the threshold quantile(RH, tau) and the new weights
        double lo = INFINITY, hi = -INFINITY;
        for (int e = tid; e < m; e += 256) { const double v = RH[e]; lo = fmin(lo, v); hi = fmax(hi, v); }
        double thresh = 0.0;
        if (uni(wg_quantile(RH, m, tau, lo, hi, &thresh))) { status = 1; break; }
        for (int e = tid; e < m; e += 256) w[e] = laa_weight(RH[e], thresh, 1e4, 1e-4);
        __syncthreads();
        ++it;
    }
    if (status) {                                                                           // the same in every thread
        if (tid == 0) { MbInfo o{}; o.status = status; o.iters = it - 1; o.score = score; a.info[b] = o; }
        return;
    }
    // ---- laa_finish: q2R.m of every node (:251-254)
    for (int v = tid; v < n; v += 256) {
        double M9[9];
        q2r(Q[v], M9);
        double* o = a.R_out + 9 * ((int64_t)no + v);
        for (int c = 0; c < 9; ++c) o[c] = M9[c];
    }
    if (tid == 0) {
        MbInfo o;
        o.iters = it - 1; o.cg_total = cg.total; o.cg_unconverged = cg.unconverged; o.status = 0; o.score = score; o.worst_sq = cg.worst_sq;
        a.info[b] = o;
    }
}

// The loop's arrays, at the handle's first loop: the incidence signs as rb_create forms them, the per-edge and per-node buffers, the
// count of edges with cycles per problem.
int mb_setup(desc_cemp_batch* h) {
    MbLoop& L = h->loop;
    const int32_t count = h->count;
    const size_t M = (size_t)h->M, N = (size_t)h->N;
    int rc;
    int8_t* d_sgn = nullptr;                           // Build_Amatrix.m:10 per CSR slot, by a launch from the set's CSR (batch_kernels.h)
    if ((rc = h->mem.alloc(&d_sgn, 2 * M))) return rc;
    hipLaunchKernelGGL(k_batch_sgn<CbProb>, dim3((unsigned)count), dim3(256), 0, h->stream, h->a.prob, h->a.rowptr, h->a.adj, d_sgn);
    DESC_HIP(hipGetLastError());
    L.sgn = d_sgn;
    if ((rc = h->mem.alloc(&L.S, M)) || (rc = h->mem.alloc(&L.R_init, 9 * N)) || (rc = h->mem.alloc(&L.R_out, 9 * N)) ||
        (rc = h->mem.alloc(&L.QQ, M)) || (rc = h->mem.alloc(&L.B, 3 * M)) || (rc = h->mem.alloc(&L.w, M)) || (rc = h->mem.alloc(&L.Res, M)) ||
        (rc = h->mem.alloc(&L.RH, M)) || (rc = h->mem.alloc(&L.info, (size_t)count)))
        return rc;
    hvec<uint8_t> hc(M);
    DESC_HIP(hipMemcpyAsync(hc.data(), h->a.has_cycle, M, hipMemcpyDeviceToHost, h->stream));
    // the largest dynamic LDS any handle may ask for: the attribute belongs to the kernel, not to a handle, so it is never lowered
    DESC_HIP(hipFuncSetAttribute((const void*)k_mpls_batch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rb_lds_bytes(REFINE_BATCH_MAX_N)));
    DESC_HIP(hipStreamSynchronize(h->stream));         // the staging vector goes out of scope below
    L.m_pos.assign((size_t)count, 0);
    for (int32_t b = 0; b < count; ++b)
        for (int64_t e = h->edge_off[(size_t)b]; e < h->edge_off[(size_t)b + 1]; ++e) L.m_pos[(size_t)b] += hc[(size_t)e] ? 1 : 0;
    L.ready = true;
    return DESC_OK;
}

int mb_run(desc_cemp_batch* h, const double* s_vec, const double* R_init, double stop_threshold, int32_t max_iter, const double* beta, int32_t n_beta,
           const double* tau, int32_t n_tau, const double* alpha, int32_t n_alpha, double* R_est, desc_mpls_info* infos, desc_mpls_batch_timings* tm) {
    auto t0 = std::chrono::steady_clock::now();
    const int32_t count = h->count;
    if (tm) { tm->ms_setup = 0; tm->ms_input = 0; tm->ms_loop = 0; tm->ms_download = 0; tm->ms_total = 0; }
    if (!beta || !tau || !alpha || n_beta < 1 || n_tau < 1 || n_alpha < 1)
        return fail(DESC_ERR_INVALID, "MPLS parameters: reweighting, thresholding and cycle_info_ratio need >= 1 entry each");
    if (count == 0) { if (tm) tm->ms_total = ms_since(t0); return DESC_OK; }
    if (!s_vec || !R_init || !R_est || !infos) return fail(DESC_ERR_INVALID, "s_vec, R_init, R_est or infos is NULL");
    int rc;
    for (int32_t b = 0; b < count; ++b) {
        const int64_t nb = h->node_off[(size_t)b + 1] - h->node_off[(size_t)b];
        if (nb > REFINE_BATCH_MAX_N)
            return fail(DESC_ERR_INVALID, "problem %d: n = %lld exceeds %d (the per-node state of the MPLS loop must fit the LDS of one workgroup): solve it with MPLS",
                        b, (long long)nb, REFINE_BATCH_MAX_N);
    }
    for (int32_t b = 0; b < count; ++b) {
        if ((rc = check_s_vec_nonneg(*h, b, s_vec))) return rc;
        for (int64_t v = h->node_off[(size_t)b]; v < h->node_off[(size_t)b + 1]; ++v)
            for (int c = 0; c < 9; ++c)
                if (!std::isfinite(R_init[9 * v + c]))
                    return fail(DESC_ERR_INVALID, "problem %d: R_init holds a non-finite entry (node %lld)", b, (long long)(v - h->node_off[(size_t)b]));
    }
    // ---- the device from here on
    DESC_HIP(hipSetDevice(h->device));
    MbLoop& L = h->loop;
    double ms_setup = 0;
    if (!L.ready) {
        auto t1 = std::chrono::steady_clock::now();
        if ((rc = mb_setup(h))) return rc;
        ms_setup = ms_since(t1);
    }
    const size_t M = (size_t)h->M, N = (size_t)h->N;
    const size_t len = (size_t)std::max(1, max_iter - 1);          // iteration it = 1 .. max_iter - 1 reads entry it - 1
    if (len > L.tab_cap) {                                          // grows only; an outgrown block stays in the arena
        const size_t cap = std::max(len, 2 * L.tab_cap);
        if ((rc = h->mem.alloc(&L.tab, 3 * cap))) return rc;
        L.tab_cap = cap;
    }
    hvec<double> tab(3 * len);
    const double* src[3] = {beta, tau, alpha};
    const int32_t cnt[3] = {n_beta, n_tau, n_alpha};
    for (int k = 0; k < 3; ++k)
        for (size_t i = 0; i < len; ++i) tab[(size_t)k * len + i] = src[k][i < (size_t)cnt[k] ? i : (size_t)cnt[k] - 1];      // padded() of mpls.hip
    DESC_HIP(hipMemcpyAsync(L.S, s_vec, sizeof(double) * M, hipMemcpyHostToDevice, h->stream));
    DESC_HIP(hipMemcpyAsync(L.R_init, R_init, sizeof(double) * 9 * N, hipMemcpyHostToDevice, h->stream));
    DESC_HIP(hipMemcpyAsync(L.tab, tab.data(), sizeof(double) * 3 * len, hipMemcpyHostToDevice, h->stream));
    DESC_HIP(hipMemsetAsync(L.info, 0xFF, sizeof(MbInfo) * (size_t)count, h->stream));      // status -1: the workgroup never finished
    DESC_HIP(hipStreamSynchronize(h->stream));          // tab goes out of use; the input's share of the wall clock
    const double ms_input = ms_since(t0) - ms_setup;
    const CbArgs& c = h->a;
    MbArgs a{};
    a.prob = c.prob; a.rowptr = c.rowptr; a.adj = c.adj; a.adj_eid = c.adj_eid; a.sgn = L.sgn; a.ii = c.ii; a.jj = c.jj; a.rij = c.rij;
    a.e_jk = c.e_jk; a.e_ki = c.e_ki; a.S0 = c.S0; a.has_cycle = c.has_cycle; a.S = L.S; a.R_init = L.R_init; a.R_out = L.R_out; a.QQ = L.QQ;
    a.B = L.B; a.w = L.w; a.Res = L.Res; a.RH = L.RH; a.info = L.info; a.beta = L.tab; a.tau = L.tab + len; a.alpha = L.tab + 2 * len;
    a.stop_threshold = stop_threshold; a.max_iter = max_iter; a.nsample = h->nsample;
    const size_t lds = rb_lds_bytes(h->max_n);
    if (lds + RB_STATIC_BYTES > (size_t)RB_LDS_BYTES) return fail(DESC_ERR_STATE, "LDS budget exceeded (%zu bytes)", lds);
    if ((rc = h->timer_begin())) return rc;
    hipLaunchKernelGGL(k_mpls_batch, dim3((unsigned)count), dim3(256), lds, h->stream, a);
    DESC_HIP(hipGetLastError());
    if ((rc = h->timer_end())) return rc;
    auto t3 = std::chrono::steady_clock::now();
    hvec<MbInfo> inf((size_t)count);
    hvec<double> R(9 * N);
    DESC_HIP(hipMemcpyAsync(inf.data(), L.info, sizeof(MbInfo) * (size_t)count, hipMemcpyDeviceToHost, h->stream));
    DESC_HIP(hipMemcpyAsync(R.data(), L.R_out, sizeof(double) * 9 * N, hipMemcpyDeviceToHost, h->stream));
    DESC_HIP(hipStreamSynchronize(h->stream));
    const double ms_wait = ms_since(t3);               // the launch and the download
    float ms = 0;
    if ((rc = h->timer_ms(&ms))) return rc;
    for (int32_t b = 0; b < count; ++b) {
        const MbInfo& g = inf[(size_t)b];
        if (g.status == 1) return fail(DESC_ERR_STATE, "problem %d: the quantile selection found no candidate (step %d)", b, (int)g.iters + 1);
        if (g.status == 2) return fail(DESC_ERR_STATE, "problem %d: the score of step %d is not finite", b, (int)g.iters + 1);
        if (g.status) return fail(DESC_ERR_STATE, "problem %d: the MPLS kernel did not finish (status %d)", b, (int)g.status);
    }
    std::memcpy(R_est, R.data(), sizeof(double) * 9 * N);
    const double ms_total = ms_since(t0);
    for (int32_t b = 0; b < count; ++b) {
        const MbInfo& g = inf[(size_t)b];
        desc_mpls_info& o = infos[b];
        o.iters = g.iters; o.cg_iters = g.cg_total; o.cg_unconverged = g.cg_unconverged; o.reserved = 0; o.m_pos = L.m_pos[(size_t)b];
        o.score = g.score; o.cg_residual = std::sqrt(g.worst_sq);           // sqrt is monotone: the largest |r|/|b| is the root of the largest ratio
        o.ms_cemp = 0; o.ms_mst = 0; o.ms_loop = ms; o.ms_total = ms_total;
    }
    if (tm) {
        tm->ms_setup = ms_setup; tm->ms_input = ms_input; tm->ms_loop = ms; tm->ms_total = ms_total;
        tm->ms_download = std::max(0.0, ms_wait - (double)ms);             // the wait for the launch is the loop's
    }
    return DESC_OK;
}

}  // namespace
}  // namespace desc

using namespace desc;

extern "C" {

int32_t desc_mpls_batch_max_n(void) { return REFINE_BATCH_MAX_N; }

int desc_mpls_batch_run(desc_cemp_batch* h, const double* s_vec, const double* R_init, double stop_threshold, int32_t max_iter,
                        const double* beta, int32_t n_beta, const double* tau, int32_t n_tau, const double* alpha, int32_t n_alpha,
                        double* R_est, desc_mpls_info* infos, desc_mpls_batch_timings* timings) {
    return no_throw("desc_mpls_batch_run", [&]() -> int {
        if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
        return mb_run(h, s_vec, R_init, stop_threshold, max_iter, beta, n_beta, tau, n_tau, alpha, n_alpha, R_est, infos, timings);
    });
}

}  // extern "C"

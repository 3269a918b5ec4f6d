// The DESC refinement tail (Algorithms/DESC.m:265-313) for many small problems in one launch (desc_refine_batch_*): the last stage of the
// "DESC" row of Demo/compare_algorithms.m for a whole Monte-Carlo batch.
//
// refine.hip runs one problem per call with a host-driven loop: seven launches per PCG step, a blocking read-back of the PCG scalars
// every 25 steps, one for the score and two or three for the quantile, 10-30 times over -- a few thousand launches and dozens of host
// round trips for a 100-node graph.  Here ONE launch refines all B problems: one workgroup of 256 threads per problem runs the whole
// loop of desc_refine_run_dev for its problem, from Q = R2Q(R_init) to q2R, without a host round trip.
//
// State.  The per-node arrays (Q, the PCG's x r z p q, rhs, diag, the vector part Wv of the update) live in LDS, 26 doubles per node.
// The LDS of a launch is sized from the largest problem of the batch; a problem addresses it with its own n, so nothing it computes
// depends on that size.  The per-edge arrays (QQ, B, w, RS and the inputs S, ii, jj, rij) lie in global memory at the problem's edge
// offset; the CSR (local ids), the endpoints and the rotations are those of the resident problem set (problem_batch.h) the handle is created
// on, and the incidence sign per slot is formed from the set's CSR by a launch in create (batch_kernels.h).
//
// Arithmetic and summation orders.  The Weighted-LAA step and the quantile are the workgroup-level functions of laa_wg.h, which
// k_mpls_batch (mpls_batch.hip) calls too.  Every per-element expression is the text of laa_math.h, which the kernels of the single path call
// too.  The single path's reductions all fit one workgroup and are reproduced in their orders: a CSR row by the 16 lanes of a DPP row
// (rhs_row16 / lap_row16), the PCG's dot products by k_cg_dot's loop and block_reduce<3, 0>, the score in 256-row chunks
// (score_chunk_sum) added in ascending order from 0.0.  The quantile's two order statistics are found exactly by a radix select over
// the 64-bit order key (8-bit digits, integer histogram in LDS); an order statistic is a value, so device_quantile's interpolation of
// them gives the same threshold.  The result is desc_refine_run's bit for bit.
//
// Control flow.  Every thread takes every decision (the stop rule, the PCG probe, the selected digit) from the same LDS values with the
// same instructions, and the integers that steer loops and barriers go through readfirstlane: the branches around the barriers are
// uniform.  Every loop is bounded by max_iters, cg_max, a row length, m or the 8 digit passes.  There is no grid-wide barrier, no
// spinning on memory, nothing between workgroups and no floating-point atomic.  A problem whose selection finds no candidate or whose
// score is not finite writes its status word and leaves.
//
// Composition independence.  Problem b's workgroup reads b's arrays and writes b's ranges; thread roles, loop bounds and summation
// orders are functions of b's n, m and CSR alone.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "batch_csr.h"
#include "batch_device.h"
#include "batch_kernels.h"
#include "problem_batch.h"
#include "laa_wg.h"

namespace desc {
namespace {

constexpr int RB_QR = 8;                               // entries of the quant_ratio table (the recurrence is constant after five steps)

// status: 0 done, 1 the selection found no candidate, 2 a score that is not finite, -1 the workgroup never finished
struct RbInfo { int32_t iters, cg_total, cg_unconverged, status; double score, worst_sq; };

struct RbArgs {
    const PbProb* prob;
    const int32_t* rowptr;      // problem b's n_b + 1 row starts at node_off[b] + b, counted inside the problem
    const int32_t* adj;         // 2 m_b local neighbour ids at 2 edge_off[b]
    const int32_t* adj_eid;     // 2 m_b local edge ids
    const int8_t* sgn;          // 2 m_b incidence signs (Build_Amatrix.m:10): -1 where the row's node is the edge's smaller endpoint
    const int32_t *ii, *jj;     // m_b local endpoints at edge_off[b]
    const double* rij;          // 9 m_b at 9 edge_off[b]
    const double* S;            // m_b at edge_off[b]
    const double* thresh0;      // per problem: max(S), the initial threshold
    const double* R_init;       // 9 n_b at 9 node_off[b]
    double* R_out;
    Quat* QQ;                   // m_b
    double *B, *w, *RS;         // 3 m_b, m_b, m_b
    RbInfo* info;
    double stop_threshold;
    int32_t max_iters;
    double qr[RB_QR];           // quant_ratio of step 1, 2, ...: the host's recurrence max(0.8, q - 0.05)
};

__global__ __launch_bounds__(256) void k_refine_batch(RbArgs a) {
    extern __shared__ double rb_lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const PbProb pd = a.prob[b];
    const int n = uni(pd.n), m = uni(pd.m);
    const int32_t* ii = a.ii + pd.edge_off;
    const int32_t* jj = a.jj + pd.edge_off;
    const double* S = a.S + pd.edge_off;
    Quat* QQ = a.QQ + pd.edge_off;
    double* B = a.B + 3 * pd.edge_off;
    double* w = a.w + pd.edge_off;
    double* RS = a.RS + pd.edge_off;
    WgLaa st;                                           // laa_wg.h: the problem's state and the step on it
    st.n = n; st.m = m;
    st.rowptr = a.rowptr + pd.node_off + b;
    st.adj = a.adj + 2 * pd.edge_off;
    st.eid = a.adj_eid + 2 * pd.edge_off;
    st.sgn = a.sgn + 2 * pd.edge_off;
    st.ii = ii; st.jj = jj; st.QQ = QQ; st.B = B; st.w = w;
    wg_laa_views(rb_lds, n, st);
    Quat* Q = st.Q;
    const double* Wv = st.Wv;

    // ---- laa_setup: Q = R2Q(R_init), QQ = R2Q(permute(RijMat, [2,1,3])); the initial weights (DESC.m:274-282)
    for (int v = tid; v < n; v += 256) Q[v] = r2q(a.R_init + 9 * (pd.node_off + v), false);
    {
        const double* rij = a.rij + 9 * pd.edge_off;
        const double thresh0 = a.thresh0[b];
        for (int e = tid; e < m; e += 256) { QQ[e] = r2q(rij + 9 * (int64_t)e, true); w[e] = laa_weight(S[e], thresh0, 1e4, 1e-4); }
    }
    __syncthreads();

    const double stop = a.stop_threshold;
    const int max_iters = a.max_iters;
    const int cg_max = min(20000, 20 * n + 200);
    double score = INFINITY;
    WgCg cg;
    int it = 1, status = 0;
    while (uni(score > stop && it < max_iters)) {                                           // DESC.m:287
        const double lam = 1.0 / (it + 1);
        score = wg_laa_step(st, cg_max, cg);                                                // Weighted_LAA
        if (uni(!isfinite(score))) { status = 2; break; }
        // ---- residuals and new weights (DESC.m:289-303)
        double lo = INFINITY, hi = -INFINITY;
        for (int e = tid; e < m; e += 256) {
            const double v = rsvec_value(Wv, B, ii, jj, S, e, lam);
            RS[e] = v; lo = fmin(lo, v); hi = fmax(hi, v);
        }
        double thresh = 0.0;
        if (uni(wg_quantile(RS, m, a.qr[min(it - 1, RB_QR - 1)], lo, hi, &thresh))) { status = 1; break; }
        for (int e = tid; e < m; e += 256) w[e] = laa_weight(RS[e], thresh, 1e4, 1e-4);
        __syncthreads();
        ++it;
    }
    const int cg_total = cg.total, cg_unconverged = cg.unconverged;
    const double worst_sq = cg.worst_sq;
    if (status) {                                                                           // the same in every thread
        if (tid == 0) { RbInfo o{}; o.status = status; o.iters = it - 1; o.score = score; a.info[b] = o; }
        return;
    }
    // ---- laa_finish: q2R.m of every node
    for (int v = tid; v < n; v += 256) {
        double M[9];
        q2r(Q[v], M);
        double* o = a.R_out + 9 * (pd.node_off + v);
        for (int c = 0; c < 9; ++c) o[c] = M[c];
    }
    if (tid == 0) {
        RbInfo o;
        o.iters = it - 1; o.cg_total = cg_total; o.cg_unconverged = cg_unconverged; o.status = 0; o.score = score; o.worst_sq = worst_sq;
        a.info[b] = o;
    }
}

}  // namespace
}  // namespace desc

using namespace desc;

struct desc_refine_batch : desc::BatchCsr, desc::BatchDevice {  // the set's offsets and endpoints; device, stream, arena, events
    const PbProb* d_prob = nullptr;
    const int32_t *d_rowptr = nullptr, *d_adj = nullptr, *d_adj_eid = nullptr, *d_ii = nullptr, *d_jj = nullptr;
    int8_t* d_sgn = nullptr;
    const double* d_rij = nullptr;
    double *d_S = nullptr, *d_thresh0 = nullptr, *d_Rinit = nullptr, *d_Rout = nullptr, *d_B = nullptr, *d_w = nullptr, *d_RS = nullptr;
    Quat* d_QQ = nullptr;
    RbInfo* d_info = nullptr;
    std::shared_ptr<desc::PbSet> set;         // the owner of d_prob, the CSR, d_ii / d_jj and d_rij
    bool own_set = false;                     // the handle made the set from a problem list and is its only owner
    ~desc_refine_batch() { close(); }         // the stream drains before the set may go
};

namespace {

int rb_check_n(int32_t b, int64_t n) {
    if (n > REFINE_BATCH_MAX_N)
        return fail(DESC_ERR_INVALID, "problem %d: n = %lld exceeds %d (the per-node state of the refinement must fit the LDS of one workgroup): solve it with DESC",
                    b, (long long)n, REFINE_BATCH_MAX_N);
    return DESC_OK;
}

// the run's own buffers
int rb_alloc_work(desc_refine_batch* h) {
    const size_t M = (size_t)h->M, N = (size_t)h->N, count = (size_t)h->count;
    int rc;
    if ((rc = h->mem.alloc(&h->d_S, M)) || (rc = h->mem.alloc(&h->d_thresh0, count)) || (rc = h->mem.alloc(&h->d_Rinit, 9 * N)) ||
        (rc = h->mem.alloc(&h->d_Rout, 9 * N)) || (rc = h->mem.alloc(&h->d_QQ, M)) || (rc = h->mem.alloc(&h->d_B, 3 * M)) ||
        (rc = h->mem.alloc(&h->d_w, M)) || (rc = h->mem.alloc(&h->d_RS, M)) || (rc = h->mem.alloc(&h->d_info, count)))
        return rc;
    // the largest dynamic LDS any handle may ask for: the attribute belongs to the kernel, not to a handle, so it is never lowered
    DESC_HIP(hipFuncSetAttribute((const void*)k_refine_batch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rb_lds_bytes(REFINE_BATCH_MAX_N)));
    return DESC_OK;
}

// The one create body, on a resident set: the caller's (desc_refine_batch_create_on, probs = NULL), or one the handle makes from probs
// and owns alone (the list path; the cap is then refused per problem inside the set's host part, between the other refusals of that
// problem).  The signs per slot come from the set's CSR in one launch (batch_kernels.h); everything else the kernel reads of the
// problems is the set's.
int rb_create(const desc_problem* probs, int32_t count, int32_t device, std::shared_ptr<PbSet> set, desc_refine_batch* h) {
    auto t0 = std::chrono::steady_clock::now();
    int rc;
    h->own_set = !set;
    if (h->own_set) {
        set = std::make_shared<PbSet>();
        if ((rc = pb_host_part(probs, count, DESC_BUILD_HOST, [](int32_t b, const desc_problem& q) -> int { return rb_check_n(b, q.n); }, set.get()))) return rc;
    } else {
        for (int32_t b = 0; b < set->count; ++b)
            if ((rc = rb_check_n(b, set->node_off[(size_t)b + 1] - set->node_off[(size_t)b]))) return rc;
    }
    h->set = set;
    pb_share_host(*set, h, !h->own_set);             // an own set: h->ii / h->jj stay EMPTY until pb_take_endpoints below -- read set->ii / set->jj till then
    h->ms_structure = ms_since(t0);
    if (h->count == 0) return DESC_OK;

    const char* what = "the batched refinement";
    if (h->own_set) {                                  // nothing above touched the device
        if ((rc = pb_device_part(probs, device, what, set.get()))) return rc;
        pb_take_endpoints(*set, h);
    }
    if ((rc = h->open(set->device, what))) return rc;
    auto t1 = std::chrono::steady_clock::now();
    h->d_prob = set->d_prob; h->d_rowptr = set->d_rowptr; h->d_adj = set->d_adj; h->d_adj_eid = set->d_adj_eid; h->d_ii = set->d_ii; h->d_jj = set->d_jj;
    h->d_rij = set->d_rij;
    if ((rc = h->mem.alloc(&h->d_sgn, 2 * (size_t)h->M))) return rc;
    hipLaunchKernelGGL(k_batch_sgn<PbProb>, dim3((unsigned)h->count), dim3(256), 0, h->stream, h->d_prob, h->d_rowptr, h->d_adj, h->d_sgn);
    DESC_HIP(hipGetLastError());
    if ((rc = rb_alloc_work(h))) return rc;
    DESC_HIP(hipStreamSynchronize(h->stream));
    h->ms_upload = ms_since(t1) + (h->own_set ? set->ms_upload : 0);
    return DESC_OK;
}

int rb_run(desc_refine_batch* h, const double* s_vec, const double* R_init, double stop_threshold, int32_t max_iters, double* R_out,
           desc_refine_info* infos, desc_refine_batch_timings* tm) {
    auto t0 = std::chrono::steady_clock::now();
    const int32_t count = h->count;
    if (tm) { tm->ms_structure = h->ms_structure; tm->ms_upload = h->ms_upload; tm->ms_input = 0; tm->ms_refine = 0; tm->ms_total = 0; }
    if (count == 0) { if (tm) tm->ms_total = ms_since(t0); return DESC_OK; }
    if (!s_vec || !R_init || !R_out || !infos) return fail(DESC_ERR_INVALID, "s_vec, R_init, R_out or infos is NULL");
    if (stop_threshold <= 0) stop_threshold = 1e-3;     // DESC.m:272
    if (max_iters <= 0) max_iters = 100;
    hvec<double> thresh0((size_t)count);                // DESC.m:274-282: quantile(S_vec, 1) = max
    int rc;
    for (int32_t b = 0; b < count; ++b) {
        if ((rc = check_s_vec_nonneg(*h, b, s_vec))) return rc;
        thresh0[(size_t)b] = *std::max_element(s_vec + h->edge_off[(size_t)b], s_vec + h->edge_off[(size_t)b + 1]);      // no problem is without edges
        for (int64_t v = h->node_off[(size_t)b]; v < h->node_off[(size_t)b + 1]; ++v)
            for (int c = 0; c < 9; ++c)
                if (!std::isfinite(R_init[9 * v + c]))
                    return fail(DESC_ERR_INVALID, "problem %d: R_init holds a non-finite entry (node %lld)", b, (long long)(v - h->node_off[(size_t)b]));
    }
    DESC_HIP(hipSetDevice(h->device));
    const size_t M = (size_t)h->M, N = (size_t)h->N;
    DESC_HIP(hipMemcpyAsync(h->d_S, s_vec, sizeof(double) * M, hipMemcpyHostToDevice, h->stream));
    DESC_HIP(hipMemcpyAsync(h->d_Rinit, R_init, sizeof(double) * 9 * N, hipMemcpyHostToDevice, h->stream));
    DESC_HIP(hipMemcpyAsync(h->d_thresh0, thresh0.data(), sizeof(double) * (size_t)count, hipMemcpyHostToDevice, h->stream));
    DESC_HIP(hipMemsetAsync(h->d_info, 0xFF, sizeof(RbInfo) * (size_t)count, h->stream));    // status -1: the workgroup never finished
    DESC_HIP(hipStreamSynchronize(h->stream));          // thresh0 goes out of use; the input's share of the wall clock
    const double ms_input = ms_since(t0);
    RbArgs a{};
    a.prob = h->d_prob; a.rowptr = h->d_rowptr; a.adj = h->d_adj; a.adj_eid = h->d_adj_eid; a.sgn = h->d_sgn; a.ii = h->d_ii; a.jj = h->d_jj;
    a.rij = h->d_rij; a.S = h->d_S; a.thresh0 = h->d_thresh0; a.R_init = h->d_Rinit; a.R_out = h->d_Rout; a.QQ = h->d_QQ; a.B = h->d_B;
    a.w = h->d_w; a.RS = h->d_RS; a.info = h->d_info; a.stop_threshold = stop_threshold; a.max_iters = max_iters;
    {
        double quant_ratio = 1.0;                       // DESC.m:296: the recurrence of desc_refine_run_dev, in the host's arithmetic
        const double quant_ratio_min = 0.8;
        for (int i = 0; i < RB_QR; ++i) { quant_ratio = std::max(quant_ratio_min, quant_ratio - 0.05); a.qr[i] = quant_ratio; }
        if (std::max(quant_ratio_min, quant_ratio - 0.05) != quant_ratio) return fail(DESC_ERR_STATE, "the quant_ratio recurrence has not settled");
    }
    const size_t lds = rb_lds_bytes(h->max_n);
    if (lds + RB_STATIC_BYTES > (size_t)RB_LDS_BYTES) return fail(DESC_ERR_STATE, "LDS budget exceeded (%zu bytes)", lds);
    if ((rc = h->timer_begin())) return rc;
    hipLaunchKernelGGL(k_refine_batch, dim3((unsigned)count), dim3(256), lds, h->stream, a);
    DESC_HIP(hipGetLastError());
    if ((rc = h->timer_end())) return rc;
    hvec<RbInfo> inf((size_t)count);
    hvec<double> R(9 * N);
    DESC_HIP(hipMemcpyAsync(inf.data(), h->d_info, sizeof(RbInfo) * (size_t)count, hipMemcpyDeviceToHost, h->stream));
    DESC_HIP(hipMemcpyAsync(R.data(), h->d_Rout, sizeof(double) * 9 * N, hipMemcpyDeviceToHost, h->stream));
    DESC_HIP(hipStreamSynchronize(h->stream));
    float ms = 0;
    if ((rc = h->timer_ms(&ms))) return rc;
    for (int32_t b = 0; b < count; ++b) {
        const RbInfo& g = inf[(size_t)b];
        if (g.status == 1) return fail(DESC_ERR_STATE, "problem %d: the quantile selection found no candidate (step %d)", b, (int)g.iters + 1);
        if (g.status == 2) return fail(DESC_ERR_STATE, "problem %d: the score of step %d is not finite", b, (int)g.iters + 1);
        if (g.status) return fail(DESC_ERR_STATE, "problem %d: the refinement kernel did not finish (status %d)", b, (int)g.status);
    }
    std::memcpy(R_out, R.data(), sizeof(double) * 9 * N);
    const double ms_total = ms_since(t0);
    for (int32_t b = 0; b < count; ++b) {
        const RbInfo& g = inf[(size_t)b];
        desc_refine_info& o = infos[b];
        o.iters = g.iters; o.cg_iters = g.cg_total; o.verbose = 0; o.cg_unconverged = g.cg_unconverged; o.score = g.score;
        o.ms_total = ms_total; o.cg_residual = std::sqrt(g.worst_sq);       // sqrt is monotone: the largest |r|/|b| is the root of the largest ratio
    }
    if (tm) { tm->ms_input = ms_input; tm->ms_refine = ms; tm->ms_total = ms_total; }
    return DESC_OK;
}

}  // namespace

extern "C" {

int32_t desc_refine_batch_max_n(void) { return REFINE_BATCH_MAX_N; }

int desc_refine_batch_create(const desc_problem* probs, int32_t count, int32_t device, desc_refine_batch** out) {
    return batch_create_guarded("desc_refine_batch_create", out, probs, count, [&](desc_refine_batch* h) { return rb_create(probs, count, device, nullptr, h); });
}

int desc_refine_batch_create_on(desc_problem_batch* set, desc_refine_batch** out) {
    return batch_create_guarded("desc_refine_batch_create_on", out, set, 0, [&](desc_refine_batch* h) { return rb_create(nullptr, 0, 0, set->s, h); }, set != nullptr);
}

int desc_refine_batch_bytes(const desc_refine_batch* h, int64_t* h2d, int64_t* d2h) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    return batch_bytes_on_set(*h, h->own_set ? h->set.get() : nullptr, h2d, d2h);
}

int desc_refine_batch_sizes(const desc_refine_batch* h, int32_t* count, int64_t* node_off, int64_t* edge_off) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    return batch_sizes(*h, count, node_off, edge_off);
}

int desc_refine_batch_run(desc_refine_batch* h, const double* s_vec, const double* R_init, double stop_threshold, int32_t max_iters,
                          double* R_out, desc_refine_info* infos, desc_refine_batch_timings* timings) {
    return no_throw("desc_refine_batch_run", [&]() -> int {
        if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
        return rb_run(h, s_vec, R_init, stop_threshold, max_iters, R_out, infos, timings);
    });
}

void desc_refine_batch_destroy(desc_refine_batch* h) { delete h; }

}  // extern "C"

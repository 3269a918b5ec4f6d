// CEMP for many small problems in one GPU pass (desc_cemp_batch_*): the baseline curve of a Monte-Carlo study next to desc_pgd_batch_*.
//
// cemp.hip solves one problem per call: the device sampler's bitmap / rank / codegree launches, a histogram read-back, allocations, the S0
// launch, max_iter round launches, one synchronise and one download -- a latency chain of a few milliseconds for a 100-node graph.  Here
// the edge lists of all B problems lie behind one another -- in the resident problem set (problem_batch.h) the handle is created on, the
// caller's or one made from the caller's problem list -- and TWO kernels walk the concatenation, one wave per edge:
//
//   k_cemp_batch_build  CEMP.m:44-103, ONE launch in create.  The wave of edge (i, j) finds its problem through a per-edge table, intersects
//                       the CSR rows of i and j in ascending k (lanes stride over the shorter row and binary-search the longer one, hits are
//                       ranked by ballot / popcount), stages the common neighbours' positions in the two rows in LDS, draws sample t as
//                       staged[desc_sample_key(seed_b, local edge id, t) mod codeg] -- desc_cemp_run's rule -- writes e_jk / e_ki as
//                       batch-global edge ids, evaluates S0 and the initial mean.  An edge without a common neighbour gets S = 1 in both
//                       ping-pong buffers and a cleared has_cycle flag.
//   k_cemp_batch_round  :107-128, max_iter launches for the whole batch.
//
// Layout.  A fixed stride of nsample slots per edge of the batch: slot (g, t) at g * nsample + t for the batch-global edge id g.  No
// compaction of the edges with cycles, no histogram, no host round trip; the rounds skip an edge whose flag is cleared.
//
// Bit-equality with desc_cemp_run.  The sampled cycles are the same (the same ascending list of common neighbours, the same key), the
// per-cycle trace product and the per-edge round are the text of cemp_math.h that cemp.hip runs, sample s sits on lane s & 63 in both,
// and the sums over lanes are group_sum<64>.
//
// Composition independence.  An edge's wave reads its own problem's rows, rotations and S values and writes its own slots; which
// workgroup runs it, how many edges the grid strides over and how much LDS the launch declares (sized from the longest row of the batch,
// addressed with the edge's own codegree) enter no result.
//
// Control flow.  No grid-wide barrier, no spinning on memory, nothing between workgroups, no atomics.  Every loop is bounded by a row
// length or nsample.  The kernels contain no workgroup barrier at all: a wave's staging area is private to it (wave barriers only).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "batch_kernels.h"
#include "cemp_batch.h"
#include "cemp_math.h"

namespace desc {
namespace {

__global__ __launch_bounds__(256) void k_cemp_batch_build(CbArgs a) {
    extern __shared__ uint32_t cb_stage[];             // per wave: lds_cap packed positions (in row i | in row j << 16) of the common neighbours
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t* st = cb_stage + (size_t)wv * a.lds_cap;
    const int nsample = a.nsample;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t g64 = wid; g64 < a.M; g64 += nw) {
        const int g = __builtin_amdgcn_readfirstlane((int)g64);
        const int b = uniform_load(a.eprob, g);
        const CbProb pd = a.prob[b];
        const int e = g - pd.edge_off;                                   // the edge's index in its problem's (i, j)-sorted list
        const int i = uniform_load(a.ii, g), j = uniform_load(a.jj, g);
        const int32_t* rp = a.rowptr + pd.node_off + b;
        const int32_t* adj = a.adj + 2 * (int64_t)pd.edge_off;
        const int32_t* eid = a.adj_eid + 2 * (int64_t)pd.edge_off;
        const int ri = uniform_load(rp, i), di = uniform_load(rp, i + 1) - ri;
        const int rj = uniform_load(rp, j), dj = uniform_load(rp, j + 1) - rj;
        const int cd = cb_common_neighbours(adj, ri, di, rj, dj, lane, a.lds_cap, st);      // :48-56, staged in ascending k
        const int64_t base = (int64_t)g * nsample;
        if (cd == 0) {                                                   // :103 SVec(~IndPosbin) = 1
            for (int t = lane; t < nsample; t += 64) { a.e_jk[base + t] = -1; a.e_ki[base + t] = -1; a.S0[base + t] = 0.0; }
            if (lane == 0) { a.S_init[g] = 1.0; a.S_a[g] = 1.0; a.S_b[g] = 1.0; a.has_cycle[g] = 0; }
            continue;
        }
        // ---- nsample draws with replacement (:57-65), S0 (:70-100) and the initial mean (:102)
        double A[9];
        load_block9(a.rij + 9 * (int64_t)g, A);
        double acc = 0.0;
        for (int s = lane; s < nsample; s += 64) {
            const uint32_t p = st[d_sample_key(pd.seed, (uint64_t)e, (uint64_t)s) % (uint64_t)cd];
            const int xi = (int)(p & 0xFFFFu), xj = (int)(p >> 16);
            const int k = adj[ri + xi];
            const int eki = pd.edge_off + eid[ri + xi], ejk = pd.edge_off + eid[rj + xj];
            double pb[9], pc[9];
            load_block9(a.rij + 9 * (int64_t)ejk, pb);
            load_block9(a.rij + 9 * (int64_t)eki, pc);
            const double d = cemp_cycle_dist(A, pb, pc, !(j < k), !(k < i));
            a.e_jk[base + s] = ejk; a.e_ki[base + s] = eki; a.S0[base + s] = d;
            acc += d;
        }
        acc = group_sum<64>(acc);
        if (lane == 0) {                                                 // :102
            const double mean = acc / (double)nsample;
            a.S_init[g] = mean; a.S_a[g] = mean; a.S_b[g] = mean; a.has_cycle[g] = 1;
        }
        __builtin_amdgcn_wave_barrier();                                 // the staging area is reused by the wave's next edge
    }
}

__global__ __launch_bounds__(256) void k_cemp_batch_round(const int32_t* e_jk, const int32_t* e_ki, const double* S0, const uint8_t* has_cycle,
                                                          const double* S_old, double* S_new, int M, int nsample, double beta) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t g = wid; g < M; g += nw) {
        if (!has_cycle[g]) continue;                                     // no cycles: SVec stays 1 (:103, :126); the same in all 64 lanes
        const double acc = cemp_edge_round(g, lane, nsample, beta, e_jk, e_ki, S0, S_old);      // cemp_math.h
        if (lane == 0) S_new[g] = acc;
    }
}

}  // namespace
}  // namespace desc

using namespace desc;

namespace {

// The sample arrays and CEMP.m:44-103 for the whole batch: the set's arrays are on the device, the handle's own are on their way there
// on its stream, t1 is when the handle's device part began.
int cb_build(desc_cemp_batch* h, std::chrono::steady_clock::time_point t1) {
    CbArgs& a = h->a;
    const int32_t nsample = h->nsample;
    const size_t M = (size_t)h->M, MC = M * (size_t)nsample;
    int rc;
    if ((rc = h->mem.alloc(&a.e_jk, MC)) || (rc = h->mem.alloc(&a.e_ki, MC)) || (rc = h->mem.alloc(&a.S0, MC)) || (rc = h->mem.alloc(&a.S_init, M)) ||
        (rc = h->mem.alloc(&a.S_a, M)) || (rc = h->mem.alloc(&a.S_b, M)) || (rc = h->mem.alloc(&a.has_cycle, M))) return rc;
    DESC_HIP(hipStreamSynchronize(h->stream));         // the caller's staging vectors may go
    h->ms_upload = ms_since(t1) + (h->own_set ? h->set->ms_upload : 0);

    // ---- CEMP.m:44-103 for the whole batch: one launch
    auto t2 = std::chrono::steady_clock::now();
    a.M = (int32_t)M; a.nsample = nsample;
    a.lds_cap = std::max(64, (h->max_deg + 63) / 64 * 64);              // the longest row bounds every codegree
    h->grid = grid_for((int64_t)M, 8192, 4);
    const size_t lds = (size_t)4 * (size_t)a.lds_cap * sizeof(uint32_t);
    if (lds > 64 * 1024) return fail(DESC_ERR_STATE, "LDS budget exceeded (%zu bytes)", lds);
    hipLaunchKernelGGL(k_cemp_batch_build, dim3((unsigned)h->grid), dim3(256), lds, h->stream, a);
    DESC_HIP(hipGetLastError());
    DESC_HIP(hipStreamSynchronize(h->stream));
    h->ms_build = ms_since(t2);
    return DESC_OK;
}

int cb_degree_refusal(int32_t b, int64_t v, int32_t d) {
    return fail(DESC_ERR_INVALID, "problem %d: node %lld has %d neighbours, more than the %d the batched sampler stages per row: solve it with CEMP",
                b, (long long)v, (int)d, CEMP_BATCH_MAX_DEGREE);
}

int cb_check_samples(const desc_cemp_batch* h, int32_t nsample) {
    if ((int64_t)h->M * nsample >= (1ll << 31))
        return fail(DESC_ERR_TOO_LARGE, "the batch holds %lld edges with %d samples each: m_total * nsample exceeds 2^31, split the batch", (long long)h->M, (int)nsample);
    return DESC_OK;
}

// The one create body, on a resident set: the caller's (desc_cemp_batch_create_on, probs = NULL), or one the handle makes from probs and
// owns alone (the list path).  The degree cap from the set's host row starts where it has them, else from a count over its host
// endpoints (a device-built CSR stays on the device); the uploads are the CbProb records; the edge -> problem map is formed by a launch
// (batch_kernels.h); the CSR, the endpoints and the rotations are the set's.
int cb_create(const desc_problem* probs, int32_t count, int32_t device, std::shared_ptr<PbSet> set, int32_t nsample, uint64_t seed, const uint64_t* seeds,
              desc_cemp_batch* h) {
    auto t0 = std::chrono::steady_clock::now();
    h->nsample = nsample;
    if (nsample < 1) return fail(DESC_ERR_INVALID, "need nsample >= 1");
    int rc;
    h->own_set = !set;
    if (h->own_set) {
        set = std::make_shared<PbSet>();
        if ((rc = pb_host_part(probs, count, DESC_BUILD_HOST, nullptr, set.get()))) return rc;
    }
    count = set->count;
    hvec<int32_t> deg;
    for (int32_t b = 0; b < count; ++b) {
        const int64_t no = set->node_off[(size_t)b], n = set->node_off[(size_t)b + 1] - no;
        const int32_t* rp = nullptr;
        if (set->host_csr) rp = set->rowptr.data() + no + b;
        else {
            deg.assign((size_t)n, 0);
            for (int64_t e = set->edge_off[(size_t)b]; e < set->edge_off[(size_t)b + 1]; ++e) { ++deg[(size_t)set->ii[(size_t)e]]; ++deg[(size_t)set->jj[(size_t)e]]; }
        }
        for (int64_t v = 0; v < n; ++v) {
            const int32_t d = rp ? rp[v + 1] - rp[v] : deg[(size_t)v];
            if (d > CEMP_BATCH_MAX_DEGREE) return cb_degree_refusal(b, v, d);
            h->max_deg = std::max(h->max_deg, d);
        }
    }
    h->set = set;
    pb_share_host(*set, h, !h->own_set);             // an own set: h->ii / h->jj stay EMPTY until pb_take_endpoints below -- read set->ii / set->jj till then
    if ((rc = cb_check_samples(h, nsample))) return rc;
    h->ms_structure = ms_since(t0);
    if (count == 0) return DESC_OK;

    const char* what = "the batched CEMP";
    if (h->own_set) {                                  // nothing above touched the device
        if ((rc = pb_device_part(probs, device, what, set.get()))) return rc;
        pb_take_endpoints(*set, h);
    }
    if ((rc = h->open(set->device, what))) return rc;
    auto t1 = std::chrono::steady_clock::now();
    hvec<CbProb> pr((size_t)count);
    for (int32_t b = 0; b < count; ++b)
        pr[(size_t)b] = CbProb{(int32_t)(set->node_off[(size_t)b + 1] - set->node_off[(size_t)b]), (int32_t)(set->edge_off[(size_t)b + 1] - set->edge_off[(size_t)b]),
                               (int32_t)set->node_off[(size_t)b], (int32_t)set->edge_off[(size_t)b], seeds ? seeds[b] : seed};
    CbArgs& a = h->a;
    int32_t* d_eprob = nullptr;
    if ((rc = h->upload(&a.prob, pr.data(), pr.size())) || (rc = h->mem.alloc(&d_eprob, (size_t)h->M))) return rc;
    hipLaunchKernelGGL(k_batch_eprob<CbProb>, dim3((unsigned)count), dim3(256), 0, h->stream, a.prob, d_eprob);
    DESC_HIP(hipGetLastError());
    a.eprob = d_eprob; a.ii = set->d_ii; a.jj = set->d_jj; a.rowptr = set->d_rowptr; a.adj = set->d_adj; a.adj_eid = set->d_adj_eid; a.rij = set->d_rij;
    return cb_build(h, t1);                            // drains the stream while pr is in scope
}

int cb_run(desc_cemp_batch* h, const double* beta, int32_t n_beta, int32_t max_iter, double* s_vec, desc_cemp_batch_timings* tm) {
    auto t0 = std::chrono::steady_clock::now();
    if (tm) { tm->ms_structure = h->ms_structure; tm->ms_upload = h->ms_upload; tm->ms_build = h->ms_build; tm->ms_rounds = 0; tm->ms_total = 0; }
    if (!beta || n_beta < 1 || max_iter < 0) return fail(DESC_ERR_INVALID, "need beta, n_beta >= 1 and max_iter >= 0");
    if (h->count == 0) { if (tm) tm->ms_total = ms_since(t0); return DESC_OK; }
    if (!s_vec) return fail(DESC_ERR_INVALID, "s_vec is NULL");
    DESC_HIP(hipSetDevice(h->device));
    const CbArgs& a = h->a;
    const size_t M = (size_t)h->M;
    // every run starts from the initial means: S_b already holds 1 where the rounds never write, and is written everywhere else before it is read
    DESC_HIP(hipMemcpyAsync(a.S_a, a.S_init, sizeof(double) * M, hipMemcpyDeviceToDevice, h->stream));
    double* S[2] = {a.S_a, a.S_b};
    int cur = 0;
    for (int it = 0; it < max_iter; ++it) {                                         // :107
        const double b = beta[it < n_beta ? it : n_beta - 1];                       // :30-34: missing betas repeat the last one
        hipLaunchKernelGGL(k_cemp_batch_round, dim3((unsigned)h->grid), dim3(256), 0, h->stream, a.e_jk, a.e_ki, a.S0, a.has_cycle, S[cur], S[cur ^ 1], a.M, a.nsample, b);
        cur ^= 1;
    }
    DESC_HIP(hipGetLastError());
    DESC_HIP(hipMemcpyAsync(s_vec, S[cur], sizeof(double) * M, hipMemcpyDeviceToHost, h->stream));
    DESC_HIP(hipStreamSynchronize(h->stream));
    if (tm) { tm->ms_rounds = ms_since(t0); tm->ms_total = tm->ms_rounds; }
    return DESC_OK;
}

}  // namespace

extern "C" {

int32_t desc_cemp_batch_max_degree(void) { return CEMP_BATCH_MAX_DEGREE; }

int desc_cemp_batch_create(const desc_problem* probs, int32_t count, int32_t nsample, uint64_t seed, const uint64_t* seeds, int32_t device,
                           desc_cemp_batch** out) {
    return batch_create_guarded("desc_cemp_batch_create", out, probs, count,
                                [&](desc_cemp_batch* h) { return cb_create(probs, count, device, nullptr, nsample, seed, seeds, h); });
}

int desc_cemp_batch_create_on(desc_problem_batch* set, int32_t nsample, uint64_t seed, const uint64_t* seeds, desc_cemp_batch** out) {
    return batch_create_guarded("desc_cemp_batch_create_on", out, set, 0,
                                [&](desc_cemp_batch* h) { return cb_create(nullptr, 0, 0, set->s, nsample, seed, seeds, h); }, set != nullptr);
}

int desc_cemp_batch_bytes(const desc_cemp_batch* h, int64_t* h2d, int64_t* d2h) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    return batch_bytes_on_set(*h, h->own_set ? h->set.get() : nullptr, h2d, d2h);
}

int desc_cemp_batch_sizes(const desc_cemp_batch* h, int32_t* count, int64_t* node_off, int64_t* edge_off) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    return batch_sizes(*h, count, node_off, edge_off);
}

int desc_cemp_batch_get_samples(desc_cemp_batch* h, int32_t* e_jk, int32_t* e_ki, double* s0, uint8_t* has_cycle) {
    return no_throw("desc_cemp_batch_get_samples", [&]() -> int {
        if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
        if (h->count == 0) return DESC_OK;
        DESC_HIP(hipSetDevice(h->device));
        const size_t M = (size_t)h->M, MC = M * (size_t)h->nsample;
        if (e_jk) DESC_HIP(hipMemcpyAsync(e_jk, h->a.e_jk, sizeof(int32_t) * MC, hipMemcpyDeviceToHost, h->stream));
        if (e_ki) DESC_HIP(hipMemcpyAsync(e_ki, h->a.e_ki, sizeof(int32_t) * MC, hipMemcpyDeviceToHost, h->stream));
        if (s0) DESC_HIP(hipMemcpyAsync(s0, h->a.S0, sizeof(double) * MC, hipMemcpyDeviceToHost, h->stream));
        if (has_cycle) DESC_HIP(hipMemcpyAsync(has_cycle, h->a.has_cycle, M, hipMemcpyDeviceToHost, h->stream));
        DESC_HIP(hipStreamSynchronize(h->stream));
        for (int32_t b = 0; b < h->count; ++b) {                         // batch-global -> local edge ids (-1 stays -1)
            const int32_t eo = (int32_t)h->edge_off[(size_t)b];
            const size_t c0 = (size_t)eo * (size_t)h->nsample, c1 = (size_t)h->edge_off[(size_t)b + 1] * (size_t)h->nsample;
            for (int32_t* q : {e_jk, e_ki}) if (q) for (size_t c = c0; c < c1; ++c) if (q[c] >= 0) q[c] -= eo;
        }
        return DESC_OK;
    });
}

int desc_cemp_batch_run(desc_cemp_batch* h, const double* beta, int32_t n_beta, int32_t max_iter, double* s_vec, desc_cemp_batch_timings* timings) {
    return no_throw("desc_cemp_batch_run", [&]() -> int {
        if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
        return cb_run(h, beta, n_beta, max_iter, s_vec, timings);
    });
}

void desc_cemp_batch_destroy(desc_cemp_batch* h) { delete h; }

}  // extern "C"

// A study's problems resident on the device across calls (desc_problem_batch_*): validation, layout and upload happen once, and the
// batched handles are created ON the set (desc_*_batch_create_on): they borrow its device arrays and upload O(B) bytes of their own.
// The list-path creates of the eigen-solve, the refinement, CEMP and IRLS make a set of their own here (pb_host_part, pb_device_part)
// and take the same way.  The generator hands its problems over without a host copy of any rotation
// (desc_problem_batch_from_models).  problem_batch.h has the layout and the ownership rule.
//
// k_pb_csr: the per-problem CSR (local ids) from the (i, j)-sorted local edge lists, element for element what batch_csr_host builds.
// One workgroup of 256 threads per problem, four phases separated by barriers; everything is integer arithmetic and no slot depends on
// the order in which anything arrives (there is no atomic):
//   A  up[v] = the first edge with ii >= v (binary search), v = 0 .. n: the edges (v, x), x > v, are the run up[v] .. up[v+1] - 1 -- the
//      larger half of row v is one contiguous run of the list.
//   B  lo[v] = the number of edges (x, v), x < v: one wave per row, lane t of a pass takes candidate x = x0 + t and looks for v in x's run
//      (binary search over jj, ascending inside a run); ballot + popcount adds the pass up.
//   C  rowptr = the exclusive prefix sums of lo[v] + (up[v+1] - up[v]) in chunks of 256 (a fixed LDS scan, integer).
//   D  one wave per row again: the same search, now the found candidates are placed at rowptr[v] + (found before me in this pass) +
//      (found in earlier passes) -- ascending x, as the host's fill in edge order gives them -- with their edge ids; then the run of A
//      is copied behind them.
// Rows of length 0 take no slot.  Cost per problem: O(n) searches over m in A, O(n^2 / 2) searches over a run (at most log2 of the
// longest run steps each) in B and again in D, O(n) in C, and 2m slots written once: for n = 100 about 10^4 short searches per phase,
// shared by 256 threads.  The kernel has no size cap: it keeps nothing in LDS but the 256 words of the scan.
// Composition independence: problem b's workgroup reads b's lists and writes b's ranges.
#include "problem_batch.h"

#include <algorithm>
#include <chrono>
#include <cstring>

namespace desc {
namespace {

// first index in [lo, hi) with a[index] >= key (a ascending there)
__device__ __forceinline__ int pb_lower_bound(const int32_t* a, int lo, int hi, int key) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// local id of the edge (x, v) in x's run [lo, hi) of jj, -1 if there is none
__device__ __forceinline__ int pb_find(const int32_t* jj, int lo, int hi, int v) {
    const int end = hi, p = pb_lower_bound(jj, lo, hi, v);
    return (p < end && jj[p] == v) ? p : -1;
}

__global__ __launch_bounds__(256) void k_pb_csr(const PbProb* prob, const int32_t* ii_all, const int32_t* jj_all, int32_t* up_all, int32_t* lo_all,
                                                int32_t* rowptr_all, int32_t* adj_all, int32_t* eid_all) {
    __shared__ int32_t scan[256];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PbProb pd = prob[b];
    const int n = pd.n, m = pd.m;
    const int32_t* ii = ii_all + pd.edge_off;
    const int32_t* jj = jj_all + pd.edge_off;
    int32_t* up = up_all + pd.node_off + b;             // n + 1 entries, as rowptr
    int32_t* lo = lo_all + pd.node_off + b;             // n entries
    int32_t* rowptr = rowptr_all + pd.node_off + b;
    int32_t* adj = adj_all + 2 * pd.edge_off;
    int32_t* eid = eid_all + 2 * pd.edge_off;

    // ---- A
    for (int v = tid; v <= n; v += 256) up[v] = v < n ? pb_lower_bound(ii, 0, m, v) : m;
    __syncthreads();
    // ---- B
    for (int v = wave; v < n; v += 4) {
        int cnt = 0;
        for (int x0 = 0; x0 < v; x0 += 64) {
            const int x = x0 + lane;
            const bool found = x < v && pb_find(jj, up[x], up[x + 1], v) >= 0;
            cnt += __popcll(__ballot(found));
        }
        if (lane == 0) lo[v] = cnt;
    }
    __syncthreads();
    // ---- C
    int carry = 0;                                      // the same in every thread
    for (int v0 = 0; v0 < n; v0 += 256) {
        const int v = v0 + tid;
        const int d = v < n ? lo[v] + (up[v + 1] - up[v]) : 0;
        scan[tid] = d;
        __syncthreads();
        for (int st = 1; st < 256; st <<= 1) {
            const int add = tid >= st ? scan[tid - st] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        if (v < n) rowptr[v] = carry + scan[tid] - d;
        carry += scan[255];
        __syncthreads();                                // scan is written again in the next chunk
    }
    if (tid == 0) rowptr[n] = carry;
    __syncthreads();
    // ---- D
    for (int v = wave; v < n; v += 4) {
        int base = rowptr[v];
        for (int x0 = 0; x0 < v; x0 += 64) {
            const int x = x0 + lane;
            const int e = x < v ? pb_find(jj, up[x], up[x + 1], v) : -1;
            const unsigned long long mk = __ballot(e >= 0);
            if (e >= 0) {
                const int slot = base + __popcll(mk & ((1ull << lane) - 1ull));
                adj[slot] = x; eid[slot] = e;
            }
            base += __popcll(mk);
        }
        const int s = up[v], c = up[v + 1] - s;
        for (int t = lane; t < c; t += 64) { adj[base + t] = jj[s + t]; eid[base + t] = s + t; }
    }
}

}  // namespace

int pb_csr_device(PbSet* s) {
    const size_t M = (size_t)s->M, NB = (size_t)s->N + (size_t)s->count;
    int32_t *d_up = nullptr, *d_lo = nullptr;
    int rc;
    if ((rc = s->mem.alloc(&s->d_rowptr, NB)) || (rc = s->mem.alloc(&s->d_adj, 2 * M)) || (rc = s->mem.alloc(&s->d_adj_eid, 2 * M)) ||
        (rc = s->mem.alloc(&d_up, NB)) || (rc = s->mem.alloc(&d_lo, NB))) return rc;
    hipLaunchKernelGGL(k_pb_csr, dim3((unsigned)s->count), dim3(256), 0, s->stream, s->d_prob, s->d_ii, s->d_jj, d_up, d_lo, s->d_rowptr, s->d_adj,
                       s->d_adj_eid);
    DESC_HIP(hipGetLastError());
    s->built_where = DESC_BUILD_DEVICE;
    return DESC_OK;
}

namespace {

// the records from the offsets, into the caller's staging vector: it lives until the caller has drained the stream
int pb_upload_prob(PbSet* s, hvec<PbProb>& pr) {
    pr.resize((size_t)s->count);
    for (int32_t b = 0; b < s->count; ++b) {
        const int64_t no = s->node_off[(size_t)b], eo = s->edge_off[(size_t)b];
        pr[(size_t)b] = PbProb{(int32_t)(s->node_off[(size_t)b + 1] - no), (int32_t)(s->edge_off[(size_t)b + 1] - eo), no, eo};
    }
    return s->upload(&s->d_prob, pr.data(), pr.size());
}

}  // namespace

int pb_host_part(const desc_problem* probs, int32_t count, int32_t csr_where, const std::function<int(int32_t, const desc_problem&)>& extra, PbSet* s) {
    auto t0 = std::chrono::steady_clock::now();
    // the words and the order of batch_csr_host in either case; the device builder needs the offsets and the endpoints only
    const int rc = csr_where == DESC_BUILD_HOST ? batch_csr_host(probs, count, extra, s) : batch_offsets_host(probs, count, extra, s);
    if (rc) return rc;
    s->host_csr = csr_where == DESC_BUILD_HOST;
    s->ms_structure = ms_since(t0);
    return DESC_OK;
}

int pb_device_part(const desc_problem* probs, int32_t device, const char* what, PbSet* s) {
    int rc = s->open(device, what);
    if (rc) return rc;
    auto t1 = std::chrono::steady_clock::now();
    const size_t M = (size_t)s->M;
    hvec<PbProb> pr;                                   // the two staging vectors live until the stream has drained, on every way out
    const hvec<double> rij = stage_rotations(probs, s->count, s->edge_off);
    rc = [&]() -> int {
        int rc;
        if ((rc = pb_upload_prob(s, pr)) || (rc = s->upload(&s->d_ii, s->ii.data(), M)) || (rc = s->upload(&s->d_jj, s->jj.data(), M)) ||
            (rc = s->upload(&s->d_rij, rij.data(), 9 * M))) return rc;
        if (!s->host_csr) return pb_csr_device(s);
        if ((rc = s->upload(&s->d_rowptr, s->rowptr.data(), s->rowptr.size())) || (rc = s->upload(&s->d_adj, s->adj.data(), 2 * M)) ||
            (rc = s->upload(&s->d_adj_eid, s->adj_eid.data(), 2 * M))) return rc;
        s->built_where = DESC_BUILD_HOST;
        return DESC_OK;
    }();
    if (rc) { (void)hipStreamSynchronize(s->stream); return rc; }
    DESC_HIP(hipStreamSynchronize(s->stream));         // from here on the arrays are read-only
    s->ms_upload = ms_since(t1);
    return DESC_OK;
}

namespace {

int pb_from_models(desc_models_batch* m, PbSet* s) {
    ModelsView v;
    int rc = models_batch_view(m, &v);
    if (rc) return rc;
    const int32_t count = v.count;
    s->count = count;
    s->node_off.assign((size_t)count + 1, 0); s->edge_off.assign((size_t)count + 1, 0);
    for (int32_t b = 0; b < count; ++b) {
        if (v.m_per[b] == 0) return fail(DESC_ERR_INVALID, "problem %d: empty edge list", b);
        s->edge_off[(size_t)b + 1] = s->edge_off[(size_t)b] + v.m_per[b];
    }
    s->M = s->edge_off[(size_t)count];
    if (s->M >= (1ll << 30))
        return fail(DESC_ERR_TOO_LARGE, "the batch holds %lld edges in total: the 2^30 index budget is exceeded, split the batch", (long long)s->M);
    if (s->M != v.M) return fail(DESC_ERR_STATE, "the generator holds %lld edges, its problems %lld", (long long)v.M, (long long)s->M);
    if (count == 0) return DESC_OK;

    if ((rc = s->open(v.device, "the resident problem set"))) return rc;
    const size_t M = (size_t)s->M;
    if ((rc = s->mem.alloc(&s->d_ii, M)) || (rc = s->mem.alloc(&s->d_jj, M)) || (rc = s->mem.alloc(&s->d_rij, 9 * M))) return rc;
    // the generator's stream has drained: one device-to-device copy each, and the models handle may go before the set
    DESC_HIP(hipMemcpyAsync(s->d_ii, v.d_ii, sizeof(int32_t) * M, hipMemcpyDeviceToDevice, s->stream));
    DESC_HIP(hipMemcpyAsync(s->d_jj, v.d_jj, sizeof(int32_t) * M, hipMemcpyDeviceToDevice, s->stream));
    DESC_HIP(hipMemcpyAsync(s->d_rij, v.d_rij, sizeof(double) * 9 * M, hipMemcpyDeviceToDevice, s->stream));
    s->ii.resize(M); s->jj.resize(M);
    if ((rc = s->download(s->ii.data(), s->d_ii, M)) || (rc = s->download(s->jj.data(), s->d_jj, M))) return rc;
    DESC_HIP(hipStreamSynchronize(s->stream));
    for (int32_t b = 0; b < count; ++b) {              // n_b = the largest endpoint + 1: what the list path's marshalling gives
        const int64_t e0 = s->edge_off[(size_t)b], e1 = s->edge_off[(size_t)b + 1];
        const int32_t n = *std::max_element(s->jj.begin() + e0, s->jj.begin() + e1) + 1;
        s->node_off[(size_t)b + 1] = s->node_off[(size_t)b] + n;
        s->max_n = std::max(s->max_n, n);
    }
    s->N = s->node_off[(size_t)count];
    hvec<PbProb> pr;
    if ((rc = pb_upload_prob(s, pr)) || (rc = pb_csr_device(s))) {
        (void)hipStreamSynchronize(s->stream);         // pr's copy may be on its way: drain before pr goes
        return rc;
    }
    DESC_HIP(hipStreamSynchronize(s->stream));
    return DESC_OK;
}

int pb_fetch(PbSet* s, int32_t* ind_i, int32_t* ind_j, double* rij, int32_t* rowptr, int32_t* adj, int32_t* adj_eid) {
    if (s->count == 0) return DESC_OK;
    const size_t M = (size_t)s->M, NB = (size_t)s->N + (size_t)s->count;
    if (ind_i) std::copy(s->ii.begin(), s->ii.end(), ind_i);
    if (ind_j) std::copy(s->jj.begin(), s->jj.end(), ind_j);
    if (s->host_csr) {
        if (rowptr) std::copy(s->rowptr.begin(), s->rowptr.end(), rowptr);
        if (adj) std::copy(s->adj.begin(), s->adj.end(), adj);
        if (adj_eid) std::copy(s->adj_eid.begin(), s->adj_eid.end(), adj_eid);
        rowptr = adj = adj_eid = nullptr;
    }
    if (!rij && !rowptr && !adj && !adj_eid) return DESC_OK;
    DESC_HIP(hipSetDevice(s->device));
    int rc;
    if (rij && (rc = s->download(rij, (const double*)s->d_rij, 9 * M))) return rc;
    if (rowptr && (rc = s->download(rowptr, (const int32_t*)s->d_rowptr, NB))) return rc;
    if (adj && (rc = s->download(adj, (const int32_t*)s->d_adj, 2 * M))) return rc;
    if (adj_eid && (rc = s->download(adj_eid, (const int32_t*)s->d_adj_eid, 2 * M))) return rc;
    DESC_HIP(hipStreamSynchronize(s->stream));
    return DESC_OK;
}

}  // namespace
}  // namespace desc

using namespace desc;

extern "C" {

int desc_problem_batch_create(const desc_problem* probs, int32_t count, int32_t device, int32_t csr_where, desc_problem_batch** out) {
    if (csr_where != DESC_BUILD_HOST && csr_where != DESC_BUILD_DEVICE) {
        if (out) *out = nullptr;
        return fail(DESC_ERR_INVALID, "csr_where = %d: need DESC_BUILD_HOST or DESC_BUILD_DEVICE", (int)csr_where);
    }
    return batch_create_guarded("desc_problem_batch_create", out, probs, count, [&](desc_problem_batch* h) {
        h->s = std::make_shared<PbSet>();
        const int rc = pb_host_part(probs, count, csr_where, nullptr, h->s.get());
        return rc || count == 0 ? rc : pb_device_part(probs, device, "the resident problem set", h->s.get());     // the host part touched no device
    });
}

int desc_problem_batch_from_models(desc_models_batch* m, desc_problem_batch** out) {
    return batch_create_guarded("desc_problem_batch_from_models", out, m, 0, [&](desc_problem_batch* h) {
        h->s = std::make_shared<PbSet>();
        return pb_from_models(m, h->s.get());
    }, m != nullptr);
}

int desc_problem_batch_sizes(const desc_problem_batch* h, int32_t* count, int64_t* node_off, int64_t* edge_off) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    return batch_sizes(*h->s, count, node_off, edge_off);
}

int desc_problem_batch_fetch(desc_problem_batch* h, int32_t* ind_i, int32_t* ind_j, double* rij, int32_t* rowptr, int32_t* adj, int32_t* adj_eid) {
    return no_throw("desc_problem_batch_fetch", [&]() -> int {
        if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
        return pb_fetch(h->s.get(), ind_i, ind_j, rij, rowptr, adj, adj_eid);
    });
}

int32_t desc_problem_batch_built_where(const desc_problem_batch* h) { return h ? h->s->built_where : (int32_t)fail(DESC_ERR_INVALID, "NULL handle"); }

int desc_problem_batch_bytes(const desc_problem_batch* h, int64_t* h2d, int64_t* d2h) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    if (h2d) *h2d = h->s->bytes_h2d;
    if (d2h) *d2h = h->s->bytes_d2h;
    return DESC_OK;
}

void desc_problem_batch_destroy(desc_problem_batch* h) { delete h; }

}  // extern "C"

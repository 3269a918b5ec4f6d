// The tree step of MPLS (Algorithms/MPLS.m:160-193) for many small problems in one launch (desc_mst_batch_*): the "CEMP+MST" row of
// Demo/compare_algorithms.m for a whole Monte-Carlo batch.
//
// mst.hip runs Boruvka on one problem with one host read-back per round.  Here ONE launch grows all B trees: one workgroup of 256
// threads per problem runs Prim from node 1 with, per node outside the tree, the lightest edge that joins it to the tree -- the pair
// (order_key(fl(S_e + 1)), edge id), mst.hip's edge order -- in LDS.  A step takes the workgroup's arg-min of those pairs under the
// lexicographic order (lanes by shuffles, the four waves through LDS), adds that node and relaxes its CSR row (every neighbour occurs
// once in a row: no two threads write the same node).  The order is total, so the minimum spanning tree is unique: Prim's tree is the
// Boruvka tree of mst_device, edge for edge.  The n - 1 edge ids go back to the host, where rooting and propagation run per problem on
// up to 16 threads with mst_device's own tail (mst_propagate).  A node's rotation is the product along its unique tree path, so it does
// not depend on the order the edges were found in: the result is mst_device's bit for bit.
//
// Control flow.  n - 1 steps, each bounded by n and a row length; the arg-min is computed by every thread from the same four LDS pairs,
// so the branches around the barriers are uniform (steering integers go through readfirstlane).  No grid-wide barrier, no spinning on
// memory, nothing between workgroups, no atomics.  A step that finds no candidate (a disconnected graph: refused on the host before
// the launch) writes the problem's status word and the workgroup leaves.  The LDS of a launch is sized from the largest problem of the
// batch; a problem addresses it with its own n.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "batch_csr.h"
#include "batch_device.h"
#include "mst_key.h"
#include "problem_batch.h"

namespace desc {
namespace {

constexpr int MST_BATCH_MAX_N = 4096;                  // 16 bytes of LDS per node: 64 KiB, what every launch may declare
static_assert(MST_BATCH_MAX_N >= 1024 && 16 * MST_BATCH_MAX_N <= 64 * 1024, "LDS budget");
constexpr int32_t MB_NONE = 0x7FFFFFFF;                // "no edge": above every edge id

struct MbProb { int32_t n, m, node_off, edge_off; };

__device__ __forceinline__ bool mb_less(unsigned long long ka, int ea, unsigned long long kb, int eb) { return ka < kb || (ka == kb && ea < eb); }

__global__ __launch_bounds__(256) void k_mst_batch(const MbProb* prob, const int32_t* rowptr_all, const int32_t* adj_all, const int32_t* eid_all,
                                                   const double* s_all, int32_t* tree_all, int32_t* status) {
    extern __shared__ unsigned long long mb_lds[];     // key[n] (8 B), then best edge[n] and in-tree flag[n] (4 B each)
    __shared__ unsigned long long r_key[4];
    __shared__ int32_t r_edge[4], r_node[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const MbProb pd = prob[b];
    const int n = __builtin_amdgcn_readfirstlane(pd.n);
    const int32_t* rowptr = rowptr_all + pd.node_off + b;
    const int32_t* adj = adj_all + 2 * (int64_t)pd.edge_off;
    const int32_t* eid = eid_all + 2 * (int64_t)pd.edge_off;
    const double* s = s_all + pd.edge_off;
    int32_t* tree = tree_all + pd.node_off - b;        // n_b - 1 ids per problem
    unsigned long long* key = mb_lds;
    int32_t* best = (int32_t*)(mb_lds + n);
    int32_t* in_tree = best + n;
    for (int v = tid; v < n; v += 256) { key[v] = ~0ull; best[v] = MB_NONE; in_tree[v] = v == 0; }      // :171 the root is node 1
    __syncthreads();
    int u = 0;                                         // the node added last
    for (int step = 0; step < n - 1; ++step) {
        // ---- relax the row of u: every neighbour outside the tree keeps the lighter of its edge and {u, v}
        const int t1 = rowptr[u + 1];
        for (int t = rowptr[u] + tid; t < t1; t += 256) {
            const int v = adj[t];
            if (in_tree[v]) continue;
            const int e = eid[t];
            const unsigned long long k = order_key(s[e] + 1.0);          // MPLS.m:162
            if (mb_less(k, e, key[v], best[v])) { key[v] = k; best[v] = e; }
        }
        __syncthreads();
        // ---- the lightest edge that leaves the tree
        unsigned long long bk = ~0ull; int be = MB_NONE, bv = -1;
        for (int v = tid; v < n; v += 256)
            if (!in_tree[v] && best[v] != MB_NONE && mb_less(key[v], best[v], bk, be)) { bk = key[v]; be = best[v]; bv = v; }
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long ok = __shfl_xor(bk, off);
            const int oe = __shfl_xor(be, off), ov = __shfl_xor(bv, off);
            if (mb_less(ok, oe, bk, be)) { bk = ok; be = oe; bv = ov; }
        }
        if (lane == 0) { r_key[wv] = bk; r_edge[wv] = be; r_node[wv] = bv; }
        __syncthreads();
        bk = r_key[0]; be = r_edge[0]; bv = r_node[0];
        for (int w = 1; w < 4; ++w) if (mb_less(r_key[w], r_edge[w], bk, be)) { bk = r_key[w]; be = r_edge[w]; bv = r_node[w]; }
        be = __builtin_amdgcn_readfirstlane(be); bv = __builtin_amdgcn_readfirstlane(bv);
        if (be == MB_NONE) {                           // no edge leaves the tree: the same in every thread
            if (tid == 0) status[b] = step + 1;
            return;
        }
        if (tid == 0) { tree[step] = be; in_tree[bv] = 1; }
        u = bv;
        __syncthreads();                               // in_tree[u] is visible, r_* are free again
    }
    if (tid == 0) status[b] = 0;
}

// desc_mst_batch_run_on: the 3 x 3 blocks of the tree's edges out of the set's rotations, for the host's rooting and propagation.  One
// workgroup per problem; thread t copies double t, t + 256, ... of the problem's 9 (n_b - 1) output doubles, so consecutive lanes store
// consecutive doubles (a wave's stores cover whole lines) and the nine lanes of a slot read its 72-byte block behind one another.  The
// loop is bounded by 9 (n_b - 1); an id outside 0 .. m_b - 1 (refused on the host before the launch) reads nothing and leaves NaN.
__global__ __launch_bounds__(256) void k_mst_gather_blocks(const MbProb* prob, const int32_t* tree_all, const double* rij_all, double* blk_all) {
    const int b = blockIdx.x;
    const MbProb pd = prob[b];
    const int32_t* tree = tree_all + pd.node_off - b;
    const double* rij = rij_all + 9 * (int64_t)pd.edge_off;
    double* blk = blk_all + 9 * (int64_t)(pd.node_off - b);
    const int total = 9 * (pd.n - 1);
    for (int q = threadIdx.x; q < total; q += 256) {
        const int slot = q / 9, c = q - 9 * slot;
        const int e = tree[slot];
        blk[q] = (unsigned)e < (unsigned)pd.m ? rij[9 * (int64_t)e + c] : __builtin_nan("");
    }
}

// connected, with every node id touched by an edge: union-find over the problem's edge list; *comps = the number of components
void mb_components(int64_t n, int64_t m, const int32_t* ii, const int32_t* jj, int64_t* comps) {
    hvec<int32_t> par((size_t)n);
    std::iota(par.begin(), par.end(), 0);
    auto find = [&](int32_t x) { while (par[x] != x) { par[x] = par[par[x]]; x = par[x]; } return x; };
    int64_t c = n;
    for (int64_t e = 0; e < m; ++e) {
        const int32_t a = find(ii[e]), b = find(jj[e]);
        if (a != b) { par[std::max(a, b)] = std::min(a, b); --c; }
    }
    *comps = c;
}

// the size cap and connectivity of one problem, from its endpoints alone
int mb_check_problem(int32_t b, int64_t n, int64_t m, const int32_t* ii, const int32_t* jj) {
    if (n > MST_BATCH_MAX_N)
        return fail(DESC_ERR_INVALID, "problem %d: n = %lld exceeds %d (the per-node keys of the tree kernel must fit the LDS of one workgroup): solve it with MST / MPLS",
                    b, (long long)n, MST_BATCH_MAX_N);
    int64_t comps = 0;
    mb_components(n, m, ii, jj, &comps);
    if (comps != 1)                                   // MPLS.m:178 would loop for ever
        return fail(DESC_ERR_INVALID, "problem %d: the graph is disconnected: %lld components (a node id in 1..max(Ind) that no edge touches is one)",
                    b, (long long)comps);
    return DESC_OK;
}

int mb_check_s_vec(const BatchCsr& h, const double* s_vec) {
    for (int32_t b = 0; b < h.count; ++b)
        for (int64_t e = h.edge_off[(size_t)b]; e < h.edge_off[(size_t)b + 1]; ++e)
            if (!std::isfinite(s_vec[e]))
                return fail(DESC_ERR_INVALID, "problem %d: S_vec entry %lld is not finite", b, (long long)(e - h.edge_off[(size_t)b]));
    return DESC_OK;
}

// validation, the size cap, connectivity, the per-problem CSR: no device.  csr = false (desc_mst_batch_check): the refusals and the
// offsets alone, and a problem may come without rotations.
int mb_host_part(const desc_problem* probs, int32_t count, const double* s_vec, BatchCsr* h, bool csr = true) {
    const auto extra = [](int32_t b, const desc_problem& q) -> int { return mb_check_problem(b, q.n, q.m, q.ind_i, q.ind_j); };
    int rc = csr ? batch_csr_host(probs, count, extra, h) : batch_offsets_host(probs, count, extra, h, false, false);
    if (rc) return rc;
    return s_vec ? mb_check_s_vec(*h, s_vec) : DESC_OK;
}

// the launch's LDS and the read-back of its status words and edge ids (into tree, N entries at least), refusing a tree that did not close
int mb_grow_trees(BatchDevice& dev, const BatchCsr& h, const MbProb* d_prob, const int32_t* d_rowptr, const int32_t* d_adj, const int32_t* d_eid,
                  const double* d_s, int32_t* d_tree, int32_t* d_status, hvec<int32_t>& tree) {
    const size_t N = (size_t)h.N, count = (size_t)h.count;
    const size_t lds = (size_t)16 * (size_t)h.max_n;
    if (lds > 64 * 1024) return fail(DESC_ERR_STATE, "LDS budget exceeded (%zu bytes)", lds);
    hipLaunchKernelGGL(k_mst_batch, dim3((unsigned)count), dim3(256), lds, dev.stream, d_prob, d_rowptr, d_adj, d_eid, d_s, d_tree, d_status);
    DESC_HIP(hipGetLastError());
    hvec<int32_t> status(count);
    tree.assign(std::max<size_t>(N, 1), 0);
    int rc;
    if ((rc = dev.download(status.data(), d_status, count))) return rc;
    if (N > count && (rc = dev.download(tree.data(), d_tree, N - count))) return rc;
    DESC_HIP(hipStreamSynchronize(dev.stream));
    for (size_t b = 0; b < count; ++b)
        if (status[b] != 0)
            return fail(DESC_ERR_STATE, "problem %d: the tree kernel found no edge leaving the tree (status %d)", (int)b, (int)status[b]);
    return DESC_OK;
}

// every edge id of problem b's tree lies in 0 .. m_b - 1
bool mb_ids_ok(const BatchCsr& h, int32_t b, const int32_t* ids) {
    const int64_t cnt = h.node_off[(size_t)b + 1] - h.node_off[(size_t)b] - 1, m = h.edge_off[(size_t)b + 1] - h.edge_off[(size_t)b];
    bool ok = true;
    for (int64_t q = 0; q < cnt; ++q) ok = ok && ids[q] >= 0 && ids[q] < m;
    return ok;
}

// On a resident set: the host part on the set's endpoint mirror, s_vec up, the tree kernel on the set's CSR, the tree's blocks gathered
// on the device (72 bytes per tree edge come down), rooting and propagation on the host as in mb_run.
int mb_run_on(const std::shared_ptr<PbSet>& set, const double* s_vec, double* R_out, int32_t* tree_edges, desc_mst_batch_timings* tm, int64_t* bytes) {
    auto t0 = std::chrono::steady_clock::now();
    if (tm) { tm->ms_structure = 0; tm->ms_upload = 0; tm->ms_tree = 0; tm->ms_propagate = 0; tm->ms_total = 0; }
    if (bytes) { bytes[0] = 0; bytes[1] = 0; }
    const BatchCsr& h = *set;
    const int32_t count = h.count;
    if (count == 0) return DESC_OK;
    if (!s_vec || !R_out) return fail(DESC_ERR_INVALID, "s_vec or R_out is NULL");
    int rc;
    for (int32_t b = 0; b < count; ++b) {
        const size_t eo = (size_t)h.edge_off[(size_t)b];
        if ((rc = mb_check_problem(b, h.node_off[(size_t)b + 1] - h.node_off[(size_t)b], h.edge_off[(size_t)b + 1] - (int64_t)eo, h.ii.data() + eo, h.jj.data() + eo)))
            return rc;
    }
    if ((rc = mb_check_s_vec(h, s_vec))) return rc;
    const double ms_structure = ms_since(t0);

    BatchDevice dev;                                   // this call's own: gone, stream drained, at every return below -- before the caller's reference to the set
    if ((rc = dev.open(set->device, "the batched tree step"))) return rc;   // nothing above touched the device
    auto t1 = std::chrono::steady_clock::now();
    const size_t M = (size_t)h.M, N = (size_t)h.N;
    hvec<MbProb> pr((size_t)count);
    for (int32_t b = 0; b < count; ++b)
        pr[(size_t)b] = MbProb{(int32_t)(h.node_off[(size_t)b + 1] - h.node_off[(size_t)b]), (int32_t)(h.edge_off[(size_t)b + 1] - h.edge_off[(size_t)b]),
                               (int32_t)h.node_off[(size_t)b], (int32_t)h.edge_off[(size_t)b]};
    MbProb* d_prob; int32_t *d_tree, *d_status; double *d_s, *d_blk;
    const size_t n_blk = 9 * (N - (size_t)count);
    if ((rc = dev.upload(&d_prob, pr.data(), pr.size())) || (rc = dev.upload(&d_s, s_vec, M)) || (rc = dev.mem.alloc(&d_tree, N)) ||
        (rc = dev.mem.alloc(&d_status, (size_t)count)) || (rc = dev.mem.alloc(&d_blk, std::max<size_t>(n_blk, 1)))) return rc;
    DESC_HIP(hipMemsetAsync(d_status, 0xFF, sizeof(int32_t) * (size_t)count, dev.stream));       // -1: the workgroup never finished
    DESC_HIP(hipStreamSynchronize(dev.stream));
    const double ms_upload = ms_since(t1);

    auto t2 = std::chrono::steady_clock::now();
    hvec<int32_t> tree;
    if ((rc = mb_grow_trees(dev, h, d_prob, set->d_rowptr, set->d_adj, set->d_adj_eid, d_s, d_tree, d_status, tree))) return rc;
    for (int32_t b = 0; b < count; ++b)                // before the gather reads rotations by these ids
        if (!mb_ids_ok(h, b, tree.data() + h.node_off[(size_t)b] - b)) return fail(DESC_ERR_STATE, "problem %d: the tree kernel's edges do not span the graph", b);
    hvec<double> blk(std::max<size_t>(n_blk, 1));
    hipLaunchKernelGGL(k_mst_gather_blocks, dim3((unsigned)count), dim3(256), 0, dev.stream, d_prob, d_tree, set->d_rij, d_blk);
    DESC_HIP(hipGetLastError());
    if ((rc = dev.download(blk.data(), d_blk, n_blk))) return rc;
    DESC_HIP(hipStreamSynchronize(dev.stream));
    const double ms_tree = ms_since(t2);

    // ---- rooting and propagation (MPLS.m:171-193) per problem on host threads: the tail of mst_device
    auto t3 = std::chrono::steady_clock::now();
    hvec<int32_t> prc((size_t)count, DESC_OK);
    for_each_problem(count, [&](int32_t b) {
        const int64_t no = h.node_off[(size_t)b], n = h.node_off[(size_t)b + 1] - no;
        const size_t eo = (size_t)h.edge_off[(size_t)b];
        int32_t* ids = tree.data() + no - b;
        const int cnt = (int)(n - 1);
        prc[(size_t)b] = mst_propagate(n, h.ii.data() + eo, h.jj.data() + eo, ids, cnt, blk.data() + 9 * (size_t)(no - b), R_out + 9 * (size_t)no);
        if (tree_edges && prc[(size_t)b] == DESC_OK) {
            std::sort(ids, ids + cnt);
            std::copy(ids, ids + cnt, tree_edges + no - b);
        }
    });
    for (int32_t b = 0; b < count; ++b)
        if (prc[(size_t)b]) return fail(DESC_ERR_STATE, "problem %d: the tree kernel's edges do not span the graph", b);
    if (tm) { tm->ms_structure = ms_structure; tm->ms_upload = ms_upload; tm->ms_tree = ms_tree; tm->ms_propagate = ms_since(t3); tm->ms_total = ms_since(t0); }
    if (bytes) { bytes[0] = dev.bytes_h2d; bytes[1] = dev.bytes_d2h; }
    return DESC_OK;
}

int mb_run(const desc_problem* probs, int32_t count, const double* s_vec, int32_t device, double* R_out, int32_t* tree_edges, desc_mst_batch_timings* tm) {
    auto t0 = std::chrono::steady_clock::now();
    if (tm) { tm->ms_structure = 0; tm->ms_upload = 0; tm->ms_tree = 0; tm->ms_propagate = 0; tm->ms_total = 0; }
    if (count == 0) return DESC_OK;
    if (!s_vec || !R_out) return fail(DESC_ERR_INVALID, "s_vec or R_out is NULL");
    BatchCsr h;
    int rc = mb_host_part(probs, count, s_vec, &h);
    if (rc) return rc;
    const double ms_structure = ms_since(t0);

    BatchDevice dev;                                   // this call's own: gone, stream drained, at every return below
    if ((rc = dev.open(device, "the batched tree step"))) return rc;        // nothing above touched the device
    auto t1 = std::chrono::steady_clock::now();
    const size_t M = (size_t)h.M, N = (size_t)h.N;
    hvec<MbProb> pr((size_t)count);
    for (int32_t b = 0; b < count; ++b) pr[(size_t)b] = MbProb{(int32_t)probs[b].n, (int32_t)probs[b].m, (int32_t)h.node_off[(size_t)b], (int32_t)h.edge_off[(size_t)b]};
    MbProb* d_prob; int32_t *d_rowptr, *d_adj, *d_eid, *d_tree, *d_status; double* d_s;
    if ((rc = dev.upload(&d_prob, pr.data(), pr.size())) || (rc = dev.upload(&d_rowptr, h.rowptr.data(), h.rowptr.size())) ||
        (rc = dev.upload(&d_adj, h.adj.data(), 2 * M)) || (rc = dev.upload(&d_eid, h.adj_eid.data(), 2 * M)) ||
        (rc = dev.upload(&d_s, s_vec, M)) || (rc = dev.mem.alloc(&d_tree, N)) || (rc = dev.mem.alloc(&d_status, (size_t)count))) return rc;
    DESC_HIP(hipMemsetAsync(d_status, 0xFF, sizeof(int32_t) * (size_t)count, dev.stream));       // -1: the workgroup never finished
    DESC_HIP(hipStreamSynchronize(dev.stream));
    const double ms_upload = ms_since(t1);

    auto t2 = std::chrono::steady_clock::now();
    hvec<int32_t> tree;
    if ((rc = mb_grow_trees(dev, h, d_prob, d_rowptr, d_adj, d_eid, d_s, d_tree, d_status, tree))) return rc;
    const double ms_tree = ms_since(t2);

    // ---- rooting and propagation (MPLS.m:171-193) per problem on host threads: the tail of mst_device
    auto t3 = std::chrono::steady_clock::now();
    hvec<int32_t> prc((size_t)count, DESC_OK);
    for_each_problem(count, [&](int32_t b) {
        const int64_t no = h.node_off[(size_t)b], n = probs[b].n;
        int32_t* ids = tree.data() + no - b;
        const int cnt = (int)(n - 1);
        bool ok = true;
        for (int q = 0; q < cnt; ++q) ok = ok && ids[q] >= 0 && ids[q] < probs[b].m;
        if (!ok) { prc[(size_t)b] = DESC_ERR_STATE; return; }
        hvec<double> blk((size_t)9 * (size_t)std::max(cnt, 1));
        for (int q = 0; q < cnt; ++q) std::memcpy(&blk[9 * (size_t)q], probs[b].rij + 9 * (size_t)ids[q], 72);
        prc[(size_t)b] = mst_propagate(n, probs[b].ind_i, probs[b].ind_j, ids, cnt, blk.data(), R_out + 9 * (size_t)no);
        if (tree_edges && prc[(size_t)b] == DESC_OK) {
            std::sort(ids, ids + cnt);
            std::copy(ids, ids + cnt, tree_edges + no - b);
        }
    });
    for (int32_t b = 0; b < count; ++b)
        if (prc[(size_t)b]) return fail(DESC_ERR_STATE, "problem %d: the tree kernel's edges do not span the graph", b);
    if (tm) { tm->ms_structure = ms_structure; tm->ms_upload = ms_upload; tm->ms_tree = ms_tree; tm->ms_propagate = ms_since(t3); tm->ms_total = ms_since(t0); }
    return DESC_OK;
}

}  // namespace
}  // namespace desc

using namespace desc;

extern "C" {

int32_t desc_mst_batch_max_n(void) { return MST_BATCH_MAX_N; }

int desc_mst_batch_check(const desc_problem* probs, int32_t count) {
    return no_throw("desc_mst_batch_check", [&]() -> int {
        if (count < 0 || (count > 0 && !probs)) return fail(DESC_ERR_INVALID, "NULL argument or negative count");
        BatchCsr h;
        return mb_host_part(probs, count, nullptr, &h, false);
    });
}

int desc_mst_batch_run_on(desc_problem_batch* set, const double* s_vec, double* R_out, int32_t* tree_edges, desc_mst_batch_timings* timings, int64_t* bytes) {
    return no_throw("desc_mst_batch_run_on", [&]() -> int {
        if (!set) return fail(DESC_ERR_INVALID, "NULL argument or negative count");
        const std::shared_ptr<PbSet> keep = set->s;   // outlives the call's device half
        return mb_run_on(keep, s_vec, R_out, tree_edges, timings, bytes);
    });
}

int desc_mst_batch_run(const desc_problem* probs, int32_t count, const double* s_vec, int32_t device, double* R_out, int32_t* tree_edges,
                       desc_mst_batch_timings* timings) {
    return no_throw("desc_mst_batch_run", [&]() -> int {
        if (count < 0 || (count > 0 && !probs)) return fail(DESC_ERR_INVALID, "NULL argument or negative count");
        return mb_run(probs, count, s_vec, device, R_out, tree_edges, timings);
    });
}

}  // extern "C"

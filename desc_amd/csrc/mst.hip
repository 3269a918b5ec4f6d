// Minimum spanning tree and rotations propagated along it: the CEMP+MST initialisation of Algorithms/MPLS.m:160-193.
//   :162      the undirected graph with edge weights SVec + 1 (the 1 keeps sparse() from dropping zero weights)
//   :166-168  minspantree
//   :171-193  root node 1 with R_1 = I; a leaf reached through edge e gets R_e * R_root when it is e's smaller endpoint i
//             (IndMat(leaf, root) > 0), R_e' * R_root otherwise
// Tree selection is Boruvka on the device CSR index of the problem.  Edge order: the computed double fl(S_e + 1.0) first -- adding
// 1 can merge values that differed -- then the edge's index in the (i, j)-sorted list.  That order is total, so the tree is unique
// and independent of the caller's row order.  MATLAB's minspantree does not document how it breaks ties; with distinct keys the
// minimum spanning tree is unique and both trees coincide.
// Per round: every CSR row takes its lexicographic minimum (key, index) over the edges that leave its component (one wave per row,
// registers and cross-lane exchanges), each component reduces its rows' minima with 64-bit atomicMin (the order-preserving bit
// pattern of the key first, the index second), mutual choices hook the higher label under the lower, and labels are flattened by
// pointer jumping.  The host drives the rounds with one read-back each, at most ceil(log2 n) + 2 of them; no device-side waits.
// Rooting and propagation run on the host (O(n), microseconds) from the n - 1 tree edges and their 72-byte blocks.
// components_device runs the same rounds with all keys equal and returns the component labels (IRLS_GM.m:65-67, irls.hip).
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "device_utils.h"
#include "mst_key.h"

namespace desc {
namespace {

constexpr int32_t NO_EDGE = 0x7F7F7F7F;           // "no edge": the byte fill of bidx (hipMemset 0x7F); above every edge index (m < 2^31)

__global__ __launch_bounds__(256) void k_mst_keys(const double* s, unsigned long long* key, int64_t m) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256) key[e] = order_key(s[e] + 1.0);   // MPLS.m:162
}
__global__ __launch_bounds__(256) void k_mst_init(int32_t* comp, int32_t* parent, int n) {
    for (int v = blockIdx.x * 256 + threadIdx.x; v < n; v += gridDim.x * 256) { comp[v] = v; parent[v] = v; }
}
// the lightest edge of row v that leaves v's component: one wave per row
__global__ __launch_bounds__(256) void k_mst_rowmin(const int32_t* rowptr, const int32_t* adj, const int32_t* eid, const int32_t* comp,
                                                    const unsigned long long* key, unsigned long long* rkey, int32_t* ridx, unsigned long long* bkey, int n) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t v = wid; v < n; v += nw) {
        const int cv = comp[v];
        unsigned long long bk = ~0ull; int bi = NO_EDGE;
        for (int t = rowptr[v] + lane; t < rowptr[v + 1]; t += 64) {
            if (comp[adj[t]] == cv) continue;
            const int e = eid[t];
            const unsigned long long k = key[e];
            if (k < bk || (k == bk && e < bi)) { bk = k; bi = e; }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long ok = __shfl_xor(bk, off);
            const int oi = __shfl_xor(bi, off);
            if (ok < bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
        }
        if (lane == 0) {
            rkey[v] = bk; ridx[v] = bi;
            if (bi != NO_EDGE) atomicMin(&bkey[cv], bk);
        }
    }
}
// the smallest index among the component's rows whose minimum has the component's key
__global__ __launch_bounds__(256) void k_mst_argmin(const int32_t* comp, const unsigned long long* rkey, const int32_t* ridx, const unsigned long long* bkey,
                                                    int32_t* bidx, int n) {
    for (int v = blockIdx.x * 256 + threadIdx.x; v < n; v += gridDim.x * 256)
        if (ridx[v] != NO_EDGE && rkey[v] == bkey[comp[v]]) atomicMin(&bidx[comp[v]], ridx[v]);
}
// every component with an outgoing edge takes it into the tree and hooks under the other end's component; of a mutual pair the lower
// label stays the root
__global__ __launch_bounds__(256) void k_mst_hook(const int32_t* comp, const int32_t* bidx, const int32_t* ii, const int32_t* jj, int32_t* parent,
                                                  uint8_t* mark, int32_t* hooked, int n) {
    for (int c = blockIdx.x * 256 + threadIdx.x; c < n; c += gridDim.x * 256) {
        if (comp[c] != c) continue;
        const int e = bidx[c];
        if (e == NO_EDGE) continue;
        const int a = comp[ii[e]], b = comp[jj[e]], d = a == c ? b : a;
        mark[e] = 1;
        if (!(bidx[d] == e && c < d)) parent[c] = d;
        atomicAdd(hooked, 1);
    }
}
// pointer jumping in place (every value read is an ancestor, so the pass only speeds up)
__global__ __launch_bounds__(256) void k_mst_jump(int32_t* parent, int n) {
    for (int v = blockIdx.x * 256 + threadIdx.x; v < n; v += gridDim.x * 256) parent[v] = parent[parent[v]];
}
__global__ __launch_bounds__(256) void k_mst_relabel(int32_t* comp, const int32_t* parent, int n) {
    for (int v = blockIdx.x * 256 + threadIdx.x; v < n; v += gridDim.x * 256) comp[v] = parent[comp[v]];
}
// the marked edges (order of arrival; the host sorts them) and their rotation blocks
__global__ __launch_bounds__(256) void k_mst_collect(const uint8_t* mark, const double* rij, int64_t m, int32_t* out, double* blocks, int32_t* count, int cap) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256) {
        if (!mark[e]) continue;
        const int p = atomicAdd(count, 1);
        if (p < cap) { out[p] = (int32_t)e; for (int q = 0; q < 9; ++q) blocks[9 * (int64_t)p + q] = rij[9 * e + q]; }
    }
}

// C = A * B, or A' * B, 3x3 column-major
void mul3(const double* A, bool transpose_a, const double* B, double* C) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double s = 0.0;
            for (int u = 0; u < 3; ++u) s += (transpose_a ? A[u + 3 * r] : A[r + 3 * u]) * B[u + 3 * c];
            C[r + 3 * c] = s;
        }
}

// The Boruvka rounds on the CSR index with edge order (d_key[e], e): on return d_comp holds every node's component label (the label of
// a component is one of its nodes) and d_mark the forest's edges (d_mark must be zeroed by the caller).  Shared by mst_device and
// components_device.
int boruvka_rounds(const desc_device_problem* dp, const unsigned long long* d_key, int32_t* d_comp, uint8_t* d_mark, DevArena& D) {
    int rc = DESC_OK;
    const int64_t n = dp->n;
    unsigned long long *d_rkey, *d_bkey;
    int32_t *d_parent, *d_ridx, *d_bidx, *d_cnt;
    if ((rc = D.alloc(&d_rkey, n)) || (rc = D.alloc(&d_bkey, n)) || (rc = D.alloc(&d_parent, n)) || (rc = D.alloc(&d_ridx, n)) ||
        (rc = D.alloc(&d_bidx, n)) || (rc = D.alloc(&d_cnt, 2)))
        return rc;
    const int ngrid = grid_for(n, 1024);
    const int wgrid = grid_for(n, 2048, 4);          // a wave per row
    hipLaunchKernelGGL(k_mst_init, dim3(ngrid), dim3(256), 0, 0, d_comp, d_parent, (int)n);
    const int log2n = (int)std::ceil(std::log2((double)n));
    const int max_rounds = log2n + 2, jumps = log2n + 1;
    for (int round = 0;; ++round) {
        if (round >= max_rounds) return fail(DESC_ERR_STATE, "minimum spanning tree: no convergence in %d rounds", max_rounds);
        DESC_HIP(hipMemsetAsync(d_bkey, 0xFF, sizeof(unsigned long long) * n, 0));
        DESC_HIP(hipMemsetAsync(d_bidx, 0x7F, sizeof(int32_t) * n, 0));                    // every entry NO_EDGE
        DESC_HIP(hipMemsetAsync(d_cnt, 0, sizeof(int32_t), 0));
        hipLaunchKernelGGL(k_mst_rowmin, dim3(wgrid), dim3(256), 0, 0, dp->d_rowptr, dp->d_adj, dp->d_adj_eid, d_comp, d_key, d_rkey, d_ridx, d_bkey, (int)n);
        hipLaunchKernelGGL(k_mst_argmin, dim3(ngrid), dim3(256), 0, 0, d_comp, d_rkey, d_ridx, d_bkey, d_bidx, (int)n);
        hipLaunchKernelGGL(k_mst_hook, dim3(ngrid), dim3(256), 0, 0, d_comp, d_bidx, dp->d_ii, dp->d_jj, d_parent, d_mark, d_cnt, (int)n);
        int32_t hooked = 0;
        DESC_HIP(hipMemcpy(&hooked, d_cnt, sizeof(int32_t), hipMemcpyDeviceToHost));
        if (hooked == 0) break;
        for (int t = 0; t < jumps; ++t) hipLaunchKernelGGL(k_mst_jump, dim3(ngrid), dim3(256), 0, 0, d_parent, (int)n);
        hipLaunchKernelGGL(k_mst_relabel, dim3(ngrid), dim3(256), 0, 0, d_comp, d_parent, (int)n);
    }
    return DESC_OK;
}

}  // namespace

int mst_propagate(int64_t n, const int32_t* ii, const int32_t* jj, const int32_t* ids, int cnt, const double* blk, double* R_out) {
    // rooting at node 1 and propagation (MPLS.m:171-193): adjacency of the tree, breadth first
    hvec<int32_t> deg((size_t)n + 1, 0), nb((size_t)2 * cnt), nbt((size_t)2 * cnt);
    for (int t = 0; t < cnt; ++t) { ++deg[ii[ids[t]] + 1]; ++deg[jj[ids[t]] + 1]; }
    for (int64_t v = 0; v < n; ++v) deg[v + 1] += deg[v];
    hvec<int32_t> fill(deg.begin(), deg.end() - 1);
    for (int t = 0; t < cnt; ++t) {
        const int a = ii[ids[t]], b = jj[ids[t]];
        nb[fill[a]] = b; nbt[fill[a]++] = t;
        nb[fill[b]] = a; nbt[fill[b]++] = t;
    }
    hvec<uint8_t> added((size_t)n, 0);
    hvec<int32_t> queue; queue.reserve((size_t)n);
    for (int q = 0; q < 9; ++q) R_out[q] = (q % 4 == 0) ? 1.0 : 0.0;                 // :174
    added[0] = 1; queue.push_back(0);
    for (size_t h = 0; h < queue.size(); ++h) {
        const int root = queue[h];
        for (int s = deg[root]; s < deg[root + 1]; ++s) {
            const int leaf = nb[s];
            if (added[leaf]) continue;
            const int t = nbt[s];
            mul3(&blk[9 * (size_t)t], leaf != ii[ids[t]], R_out + 9 * (int64_t)root, R_out + 9 * (int64_t)leaf);     // :184-188
            added[leaf] = 1; queue.push_back(leaf);
        }
    }
    if ((int64_t)queue.size() != n) return fail(DESC_ERR_STATE, "minimum spanning tree does not span the graph");
    return DESC_OK;
}

int mst_device(const desc_device_problem* dp, const double* d_s, double* R_out, int32_t* tree_edges) {
    int rc = DESC_OK;
    const int64_t n = dp->n, m = dp->m;
    if (n <= 0) return fail(DESC_ERR_INVALID, "empty graph");
    DevArena D;
    unsigned long long* d_key;
    int32_t *d_comp, *d_cnt, *d_ids;
    uint8_t* d_mark;
    double* d_blocks;
    if ((rc = D.alloc(&d_key, m)) || (rc = D.alloc(&d_comp, n)) || (rc = D.alloc(&d_cnt, 2)) || (rc = D.alloc(&d_ids, n)) ||
        (rc = D.alloc(&d_mark, m)) || (rc = D.alloc(&d_blocks, 9 * n)))
        return rc;
    const int egrid = grid_for(m, 2048);
    if (m) {
        hipLaunchKernelGGL(k_mst_keys, dim3(egrid), dim3(256), 0, 0, d_s, d_key, m);
        DESC_HIP(hipMemsetAsync(d_mark, 0, m, 0));
    }
    if ((rc = boruvka_rounds(dp, d_key, d_comp, d_mark, D))) return rc;
    DESC_HIP(hipMemsetAsync(d_cnt, 0, sizeof(int32_t), 0));
    if (m) hipLaunchKernelGGL(k_mst_collect, dim3(egrid), dim3(256), 0, 0, d_mark, dp->d_rij, m, d_ids, d_blocks, d_cnt, (int)n);
    DESC_HIP(hipGetLastError());
    int32_t cnt = 0;
    DESC_HIP(hipMemcpy(&cnt, d_cnt, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (cnt > n - 1) return fail(DESC_ERR_STATE, "minimum spanning tree: %d edges for %lld nodes", cnt, (long long)n);
    if (cnt < n - 1)                      // a forest: MPLS.m:178 would loop for ever
        return fail(DESC_ERR_INVALID, "the graph is disconnected: %lld components (a node id in 1..max(Ind) that no edge touches is one)",
                    (long long)(n - cnt));
    hvec<int32_t> ids((size_t)cnt);
    hvec<double> blk((size_t)9 * cnt);
    if (cnt) {
        DESC_HIP(hipMemcpy(ids.data(), d_ids, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost));
        DESC_HIP(hipMemcpy(blk.data(), d_blocks, sizeof(double) * 9 * cnt, hipMemcpyDeviceToHost));
    }
    if ((rc = mst_propagate(n, dp->ii.data(), dp->jj.data(), ids.data(), cnt, blk.data(), R_out))) return rc;
    if (tree_edges) {
        std::sort(ids.begin(), ids.end());
        std::copy(ids.begin(), ids.end(), tree_edges);
    }
    return DESC_OK;
}

int components_device(const desc_device_problem* dp, int32_t* comp_out, int64_t* count) {
    int rc = DESC_OK;
    const int64_t n = dp->n, m = dp->m;
    if (n <= 0) return fail(DESC_ERR_INVALID, "empty graph");
    DevArena D;
    unsigned long long* d_key;
    int32_t* d_comp;
    uint8_t* d_mark;
    if ((rc = D.alloc(&d_key, m)) || (rc = D.alloc(&d_comp, n)) || (rc = D.alloc(&d_mark, m))) return rc;
    if (m) {                                                          // all keys equal: the edge index decides, any forest will do
        DESC_HIP(hipMemsetAsync(d_key, 0, sizeof(unsigned long long) * m, 0));
        DESC_HIP(hipMemsetAsync(d_mark, 0, m, 0));
    }
    if ((rc = boruvka_rounds(dp, d_key, d_comp, d_mark, D))) return rc;
    DESC_HIP(hipGetLastError());
    DESC_HIP(hipMemcpy(comp_out, d_comp, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    hvec<uint8_t> seen((size_t)n, 0);
    int64_t c = 0;
    for (int64_t v = 0; v < n; ++v) {
        const int32_t l = comp_out[v];
        if (l < 0 || l >= n) return fail(DESC_ERR_STATE, "component labelling: label %d out of range", (int)l);
        if (!seen[l]) { seen[l] = 1; ++c; }
    }
    *count = c;
    return DESC_OK;
}

}  // namespace desc

using namespace desc;

extern "C" int desc_mst_run(const desc_problem* prob, const double* s_vec, int32_t device, double* R_out, int32_t* tree_edges) {
    if (!prob || !s_vec || !R_out) return fail(DESC_ERR_INVALID, "NULL argument");
    return with_uploaded(prob, device, [&](const desc_device_problem* dp) { return desc_mst_run_dev(dp, s_vec, R_out, tree_edges); });
}

extern "C" int desc_mst_run_dev(const desc_device_problem* dp, const double* s_vec, double* R_out, int32_t* tree_edges) {
    return no_throw("desc_mst_run_dev", [&]() -> int {
    if (!dp || !s_vec || !R_out) return fail(DESC_ERR_INVALID, "NULL argument");
    DESC_HIP(hipSetDevice(dp->device));
    DevArena A;
    double* d_s = nullptr;
    int rc = A.alloc(&d_s, dp->m);
    if (rc) return rc;
    if (dp->m) DESC_HIP(hipMemcpy(d_s, s_vec, sizeof(double) * dp->m, hipMemcpyHostToDevice));
    return mst_device(dp, d_s, R_out, tree_edges);
    });
}

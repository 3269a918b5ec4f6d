// Host part shared by the batched calls that walk per-problem CSR rows: validation, offsets and the CSR of every problem with LOCAL node
// and edge ids -- what desc_gcw_batch_csr returns -- and the host loops every batched call repeats.  No device: the device half of a
// handle is BatchDevice (batch_device.h).  The builders are called by the resident problem set (problem_batch.hip: the eigen-solve, the
// refinement, CEMP with MPLS and IRLS are created on a set and call none themselves) and by the calls that stay off a set:
// mst_batch.hip, lp_batch.hip, batch_structure.hip.
#pragma once
#include <cmath>
#include <cstring>
#include <functional>

#include "common.h"

namespace desc {

struct BatchCsr {
    int32_t count = 0, max_n = 0;
    hvec<int64_t> node_off, edge_off;
    hvec<int32_t> ii, jj;                     // local endpoints of every problem behind one another (host checks, the refusal's node)
    hvec<int32_t> rowptr, adj, adj_eid;       // per-problem CSR, local ids: rowptr of problem b at node_off[b] + b; filled by batch_csr_host
                                              // alone -- a handle on a set (pb_share_host) leaves them empty
    int64_t N = 0, M = 0;
};

// Refuses -- naming the problem -- what validate_problem refuses, an empty edge list, what `extra` (nullable: the caller's own caps,
// called per problem after those two) refuses, and a batch of 2^30 edges or more.  allow_empty: a problem without an edge is taken
// (rows of length 0), for the caller whose host path takes it (batch_structure.hip).  Defined in gcw_batch.hip.
int batch_csr_host(const desc_problem* probs, int32_t count, const std::function<int(int32_t, const desc_problem&)>& extra, BatchCsr* h,
                   bool allow_empty = false);
// The first half of batch_csr_host alone -- its refusals in its order, the offsets, ii and jj -- for the caller whose CSR is built on
// the device (problem_batch.hip), and, with need_rij = false, for the check that reads no rotation (desc_mst_batch_check).  Defined in
// gcw_batch.hip.
int batch_offsets_host(const desc_problem* probs, int32_t count, const std::function<int(int32_t, const desc_problem&)>& extra, BatchCsr* h,
                       bool allow_empty = false, bool need_rij = true);

// fn(b) for every problem, the problems dealt round-robin to 16 host threads at most (run_threads: exceptions reach the caller)
template <class F>
void for_each_problem(int32_t count, F&& fn) {
    const int T = std::max(1, std::min(count, 16));
    run_threads(T, [&](int t) { for (int32_t b = t; b < count; b += T) fn(b); });
}

// the body of every desc_*_batch_sizes with node and edge offsets
inline int batch_sizes(const BatchCsr& h, int32_t* count, int64_t* node_off, int64_t* edge_off) {
    if (count) *count = h.count;
    if (node_off) std::copy(h.node_off.begin(), h.node_off.end(), node_off);
    if (edge_off) std::copy(h.edge_off.begin(), h.edge_off.end(), edge_off);
    return DESC_OK;
}

// all rotations of a batch behind one another, for one host -> device copy: problem b's 9 m_b doubles at 9 * edge_off[b]
inline hvec<double> stage_rotations(const desc_problem* probs, int32_t count, const hvec<int64_t>& edge_off) {
    hvec<double> rij(9 * (size_t)edge_off[(size_t)count]);
    for (int32_t b = 0; b < count; ++b)
        if (probs[b].m) std::memcpy(rij.data() + 9 * (size_t)edge_off[(size_t)b], probs[b].rij, sizeof(double) * 9 * (size_t)probs[b].m);
    return rij;
}

// Problem b's share of a batch-long S_vec: the single calls refuse what makes a weighted degree non-finite, naming the node; here the
// entries themselves are checked.  Per problem, so that a caller's other per-problem refusals keep their place in the order.
inline int check_s_vec_nonneg(const BatchCsr& h, int32_t b, const double* s_vec) {
    for (int64_t e = h.edge_off[(size_t)b]; e < h.edge_off[(size_t)b + 1]; ++e)
        if (!(s_vec[e] >= 0) || !std::isfinite(s_vec[e]))
            return fail(DESC_ERR_INVALID, "problem %d: S_vec holds a negative or non-finite entry (node %d)", b, (int)h.ii[(size_t)e]);
    return DESC_OK;
}

}  // namespace desc

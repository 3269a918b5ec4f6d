// What a handle on a resident problem set (problem_batch.h) derives from the set's arrays by a launch in create: the edge -> problem map
// (batch_structure.hip, cemp_batch.hip, irls_batch.hip) and the incidence sign per CSR slot (refine_batch.hip, mpls_batch.hip,
// irls_batch.hip).  One text each; no host pass forms them.  P is the caller's problem record: n, m, node_off, edge_off (PbProb, CbProb).
// One workgroup of 256 threads per problem; every loop is bounded by m_b, n_b or a row length; integers only, no barrier, no atomics,
// nothing between workgroups.  Problem b's workgroup writes b's ranges alone.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace desc {

// eprob[edge_off[b] + e] = b for the m_b edges of problem b
template <class P>
__global__ __launch_bounds__(256) void k_batch_eprob(const P* prob, int32_t* eprob) {
    const int b = blockIdx.x;
    const P pd = prob[b];
    for (int e = threadIdx.x; e < pd.m; e += 256) eprob[pd.edge_off + e] = b;
}

// Build_Amatrix.m:10 per CSR slot, for rb_create, mb_setup and ib_create: -1 where the row's node is the edge's smaller endpoint, +1 at
// the larger.  A thread per row.
template <class P>
__global__ __launch_bounds__(256) void k_batch_sgn(const P* prob, const int32_t* rowptr_all, const int32_t* adj_all, int8_t* sgn_all) {
    const int b = blockIdx.x;
    const P pd = prob[b];
    const int32_t* rowptr = rowptr_all + pd.node_off + b;
    const int32_t* adj = adj_all + 2 * (int64_t)pd.edge_off;
    int8_t* sgn = sgn_all + 2 * (int64_t)pd.edge_off;
    for (int v = threadIdx.x; v < pd.n; v += 256)
        for (int t = rowptr[v]; t < rowptr[v + 1]; ++t) sgn[t] = v < adj[t] ? -1 : +1;
}

}  // namespace desc

// Host part shared by the batched calls that walk per-problem CSR rows (gcw_batch.hip, cemp_batch.hip, mst_batch.hip): validation,
// offsets and the CSR of every problem with LOCAL node and edge ids -- what desc_gcw_batch_csr returns.  No device.
#pragma once
#include <functional>

#include "common.h"

namespace desc {

struct BatchCsr {
    int32_t count = 0, max_n = 0;
    hvec<int64_t> node_off, edge_off;
    hvec<int32_t> ii, jj;                     // local endpoints of every problem behind one another (host checks, the refusal's node)
    hvec<int32_t> rowptr, adj, adj_eid;       // per-problem CSR, local ids: rowptr of problem b at node_off[b] + b
    int64_t N = 0, M = 0;
};

// Refuses -- naming the problem -- what validate_problem refuses, an empty edge list, what `extra` (nullable: the caller's own caps,
// called per problem after those two) refuses, and a batch of 2^30 edges or more.  Defined in gcw_batch.hip.
int batch_csr_host(const desc_problem* probs, int32_t count, const std::function<int(int32_t, const desc_problem&)>& extra, BatchCsr* h);

}  // namespace desc

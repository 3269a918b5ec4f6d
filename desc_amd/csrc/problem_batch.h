// A problem set resident on the device (desc_problem_batch_*, problem_batch.hip): the problems of B independent instances, validated,
// laid out and uploaded ONCE, for every batched handle that is created on it (desc_gcw_batch_create_on, desc_refine_batch_create_on,
// desc_pgd_batch_create_on, desc_cemp_batch_create_on, desc_irls_batch_create_on) and for desc_mst_batch_run_on.  The layout is the one the batched handles make for themselves (batch_csr.h): problem b's rowptr at
// node_off[b] + b, its adj / adj_eid at 2 edge_off[b], its rij at 9 edge_off[b], local ids throughout.
//
// Ownership.  The C handle holds a shared_ptr to the set; a handle created on the set holds another.  desc_problem_batch_destroy drops
// the caller's; the device blocks go back to the cache with the last owner.  After create the device arrays are read-only and the set's
// stream has drained, so any stream of the same device may read them without an event.
#pragma once
#include <memory>

#include "batch_csr.h"
#include "batch_device.h"

namespace desc {

struct PbProb { int32_t n, m; int64_t node_off, edge_off; };      // the record of GbProb and RbProb: n_b, m_b and the two offsets

struct PbSet : BatchCsr, BatchDevice {
    // BatchCsr: count, max_n, node_off, edge_off, ii, jj always; rowptr, adj, adj_eid only where the host builder made them (host_csr)
    bool host_csr = false;
    int32_t built_where = DESC_BUILD_HOST;
    PbProb* d_prob = nullptr;
    int32_t *d_ii = nullptr, *d_jj = nullptr, *d_rowptr = nullptr, *d_adj = nullptr, *d_adj_eid = nullptr;
    double* d_rij = nullptr;
    ~PbSet() { close(); }
};

// The batch CSR on the device (k_pb_csr): rowptr, adj, adj_eid of every problem from the sorted local edge lists d_ii / d_jj, element
// for element batch_csr_host's.  Allocates the three arrays in s->mem; uploads O(B) bytes; returns with the launch queued on s->stream.
int pb_csr_device(PbSet* s);

// For a create_on: the set's host offsets and endpoints into a handle's BatchCsr base (its run checks read them); the CSR stays on the
// device.
inline void pb_share_host(const PbSet& s, BatchCsr* h) {
    h->count = s.count; h->max_n = s.max_n; h->node_off = s.node_off; h->edge_off = s.edge_off; h->ii = s.ii; h->jj = s.jj;
    h->N = s.N; h->M = s.M;
}

// What desc_problem_batch_from_models takes from a generator handle (models_batch.hip): the node and edge passes have run, the
// generator's stream has drained.  Pointers into the generator's arena, valid while it lives.
struct ModelsView {
    int32_t count = 0, device = 0;
    const int64_t* m_per = nullptr;           // count
    const int32_t *d_ii = nullptr, *d_jj = nullptr;
    const double* d_rij = nullptr;
    int64_t M = 0;
};

}  // namespace desc

struct desc_problem_batch { std::shared_ptr<desc::PbSet> s; };

namespace desc {
int models_batch_view(desc_models_batch* m, ModelsView* out);
}

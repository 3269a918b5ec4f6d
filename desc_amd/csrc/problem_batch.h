// A problem set resident on the device (desc_problem_batch_*, problem_batch.hip): the problems of B independent instances, validated,
// laid out and uploaded ONCE, for every batched handle that is created on it (desc_gcw_batch_create_on, desc_refine_batch_create_on,
// desc_pgd_batch_create_on, desc_cemp_batch_create_on, desc_irls_batch_create_on) and for desc_mst_batch_run_on.  Problem b's rowptr
// lies at node_off[b] + b, its adj / adj_eid at 2 edge_off[b], its rij at 9 edge_off[b], local ids throughout.  The eigen-solve, the
// refinement, CEMP (with MPLS) and IRLS have no layout of their own: created from a problem list, a handle first makes a set from the
// list (pb_host_part, pb_device_part) and is then created on it like any other.
//
// Ownership.  The set lives behind a shared_ptr.  The C handle desc_problem_batch holds one; a handle created on the set holds another,
// and desc_problem_batch_destroy drops the caller's.  A handle created from a problem list is the only owner of the set it made.  The
// device blocks go back to the cache with the last owner.  After create the device arrays are read-only and the set's stream has
// drained, so any stream of the same device may read them without an event.
#pragma once
#include <memory>

#include "batch_csr.h"
#include "batch_device.h"

namespace desc {

struct PbProb { int32_t n, m; int64_t node_off, edge_off; };      // n_b, m_b and the two offsets: the record every kernel on a set reads

struct PbSet : BatchCsr, BatchDevice {
    // BatchCsr: count, max_n, node_off, edge_off, ii, jj always; rowptr, adj, adj_eid only where the host builder made them (host_csr)
    bool host_csr = false;
    int32_t built_where = DESC_BUILD_HOST;
    PbProb* d_prob = nullptr;
    int32_t *d_ii = nullptr, *d_jj = nullptr, *d_rowptr = nullptr, *d_adj = nullptr, *d_adj_eid = nullptr;
    double* d_rij = nullptr;
    ~PbSet() { close(); }
};

// A set in two parts, so that a handle that makes its own can run its host refusals between them: nothing touches the device before the
// last host refusal.
// Host part: what batch_csr_host refuses, in its order and words (`extra`, nullable, is the caller's per-problem cap), the offsets, ii
// and jj and, for DESC_BUILD_HOST, the CSR.  No HIP call.
int pb_host_part(const desc_problem* probs, int32_t count, int32_t csr_where, const std::function<int(int32_t, const desc_problem&)>& extra, PbSet* s);
// Device part, after the host part of the same problems: opens the device -- `what` names the call in the refusal of a machine without
// one (BatchDevice::open) --, uploads the records, the endpoints, the rotations and the CSR (or builds it there), drains the stream.
int pb_device_part(const desc_problem* probs, int32_t device, const char* what, PbSet* s);

// The batch CSR on the device (k_pb_csr): rowptr, adj, adj_eid of every problem from the sorted local edge lists d_ii / d_jj, element
// for element batch_csr_host's.  Allocates the three arrays in s->mem; uploads O(B) bytes; returns with the launch queued on s->stream.
int pb_csr_device(PbSet* s);

// For a handle on the set: the set's host offsets and, with `endpoints`, a copy of its endpoints into the handle's BatchCsr base (its run
// checks read them); the CSR stays on the device.  A handle that made the set takes the endpoints instead, once the set's device part
// has uploaded them: it is the only owner, nobody will read the set's.
inline void pb_share_host(const PbSet& s, BatchCsr* h, bool endpoints) {
    h->count = s.count; h->max_n = s.max_n; h->node_off = s.node_off; h->edge_off = s.edge_off; h->N = s.N; h->M = s.M;
    if (endpoints) { h->ii = s.ii; h->jj = s.jj; }
}
inline void pb_take_endpoints(PbSet& s, BatchCsr* h) { h->ii = std::move(s.ii); h->jj = std::move(s.jj); }

// The body of desc_*_batch_bytes of a handle on a set: the handle's counters, and the set's with them where the handle made the set
// (own: the caller never saw it); a set of the caller's reports its own (desc_problem_batch_bytes).
inline int batch_bytes_on_set(const BatchDevice& h, const PbSet* own, int64_t* h2d, int64_t* d2h) {
    if (h2d) *h2d = h.bytes_h2d + (own ? own->bytes_h2d : 0);
    if (d2h) *d2h = h.bytes_d2h + (own ? own->bytes_d2h : 0);
    return DESC_OK;
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

// The batched CEMP handle as its two users see it: cemp_batch.hip (sampling, S0, the rounds) and mpls_batch.hip (the MPLS loop on the
// resident samples).  Internal; the C ABI keeps desc_cemp_batch opaque.
#pragma once
#include "batch_csr.h"
#include "batch_device.h"
#include "laa_math.h"

namespace desc {

struct CbProb { int32_t n, m, node_off, edge_off; uint64_t seed; };

struct CbArgs {
    const CbProb* prob;
    const int32_t* eprob;       // batch-global edge id -> problem
    const int32_t* ii;          // local endpoints of every edge
    const int32_t* jj;
    const int32_t* rowptr;      // problem b's n_b + 1 row starts at node_off[b] + b, counted inside the problem
    const int32_t* adj;         // 2 m_b local neighbour ids at 2 edge_off[b]
    const int32_t* adj_eid;     // 2 m_b local edge ids
    const double* rij;          // 9 per edge
    int32_t* e_jk;              // M * nsample batch-global edge ids (-1: the edge has no cycle)
    int32_t* e_ki;
    double* S0;                 // M * nsample
    double* S_init;             // M: the initial means (:102-103), kept for the next run of the handle
    double* S_a;                // M: the ping-pong buffers of the rounds
    double* S_b;
    uint8_t* has_cycle;         // M
    int32_t M, nsample, lds_cap;
};

// status: 0 done, 1 the selection found no candidate, 2 a score that is not finite, -1 the workgroup never finished
struct MbInfo { int32_t iters, cg_total, cg_unconverged, status; double score, worst_sq; };

// what desc_mpls_batch_run adds to the handle at its first call (mpls_batch.hip)
struct MbLoop {
    bool ready = false;
    const int8_t* sgn = nullptr;        // 2 m_b incidence signs (Build_Amatrix.m:10) per CSR slot
    double *S = nullptr, *R_init = nullptr, *R_out = nullptr, *B = nullptr, *w = nullptr, *Res = nullptr, *RH = nullptr;
    Quat* QQ = nullptr;
    MbInfo* info = nullptr;
    double* tab = nullptr;              // beta | tau | alpha, tab_cap entries each
    size_t tab_cap = 0;
    hvec<int64_t> m_pos;                // per problem: its edges with a 3-cycle
};

}  // namespace desc

struct desc_cemp_batch : desc::BatchCsr, desc::BatchDevice {
    int32_t nsample = 0, max_deg = 0, grid = 1;
    desc::CbArgs a{};
    double ms_build = 0;
    desc::MbLoop loop;
};

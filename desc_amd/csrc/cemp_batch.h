// The batched CEMP handle as its two users see it: cemp_batch.hip (sampling, S0, the rounds) and mpls_batch.hip (the MPLS loop on the
// resident samples).  Internal; the C ABI keeps desc_cemp_batch opaque.
#pragma once
#include "batch_csr.h"
#include "batch_device.h"
#include "laa_math.h"
#include "problem_batch.h"

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

constexpr int CEMP_BATCH_MAX_DEGREE = 4096;            // longest CSR row: 4 waves x 4096 staged positions x 4 B = the 64 KiB every launch may declare
static_assert(CEMP_BATCH_MAX_DEGREE >= 512 && CEMP_BATCH_MAX_DEGREE <= 65536, "row positions are packed in 16 bits each");
static_assert(4 * CEMP_BATCH_MAX_DEGREE * 4 <= 64 * 1024, "LDS budget");

// The common neighbours of i and j in ascending k (CEMP.m:48-56), by one wave: lanes stride over the shorter of the two CSR rows (ri, di /
// rj, dj: start and length in adj) and binary-search the longer one, hits are ranked by ballot / popcount.  st[0 .. min(cd, lds_cap)) gets
// the positions of the hits in the two rows, packed (in row i | in row j << 16); returns the codegree cd, the same in every lane.  Ends
// with a wave barrier: st is the wave's own staging area.
__device__ __forceinline__ int cb_common_neighbours(const int32_t* adj, int ri, int di, int rj, int dj, int lane, int lds_cap, uint32_t* st) {
    const bool i_short = di <= dj;
    const int rs = i_short ? ri : rj, ds = i_short ? di : dj, rl = i_short ? rj : ri, dl = i_short ? dj : di;
    int cd = 0;
    for (int t0 = 0; t0 < ds; t0 += 64) {
        const int t = t0 + lane;
        bool hit = false;
        int lo = 0;
        if (t < ds) {
            const int k = adj[rs + t];
            int hi = dl;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (adj[rl + mid] < k) lo = mid + 1; else hi = mid; }
            hit = lo < dl && adj[rl + lo] == k;
        }
        const unsigned long long mk = __ballot(hit);
        const int pos = cd + __popcll(mk & ((1ull << lane) - 1ull));
        if (hit && pos < lds_cap) st[pos] = i_short ? ((uint32_t)t | (uint32_t)lo << 16) : ((uint32_t)lo | (uint32_t)t << 16);
        cd += __popcll(mk);
    }
    cd = __builtin_amdgcn_readfirstlane(cd);
    __builtin_amdgcn_wave_barrier();
    return cd;
}

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
    std::shared_ptr<desc::PbSet> set;         // the owner of the CSR, a.ii / a.jj and a.rij
    bool own_set = false;                     // the handle made the set from a problem list and is its only owner
    ~desc_cemp_batch() { close(); }           // the stream drains before the set may go
};

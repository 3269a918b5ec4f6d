// Internal: CEMP's sampled cycles and their S0 kept on the device between the two steps of Algorithms/CEMP.m (build + S0Mat :44-103,
// rounds :107-128), so that MPLS (Algorithms/MPLS.m:65-158, the same lines) can re-use them in its loop (:223-237).  Kernels in cemp.hip.
#pragma once
#include "device_utils.h"

namespace desc {

struct CempState : DevArena {                             // owns its device blocks
    int64_t n = 0, m = 0, mp = 0, mc = 0;                 // nodes, edges, edges with cycles, mp * nsample
    int32_t nsample = 0, max_deg = 0;
    bool tiles = false;                                   // the rounds run on the CSR-aligned copy in tiles (k_cemp_round_tile)
    int32_t *d_pos = nullptr, *d_k = nullptr, *d_ejk = nullptr, *d_eki = nullptr;   // samples (CoIndMat and its two edge ids)
    uint32_t* d_pk = nullptr;                             // packed row positions of k (tile path)
    double* d_S0 = nullptr;                               // S0Mat, mc entries
    double* d_S[2] = {nullptr, nullptr};                  // SVec (CSR-aligned, 2m, on the tile path; edge-indexed otherwise), ping-pong
    int cur = 0;
    int32_t *d_slot_a = nullptr, *d_slot_b = nullptr;     // slots of every edge in its two CSR rows (tile path)
    int32_t* d_poe = nullptr;                             // edge -> index among the edges with cycles, -1 without (NULL: identity)
    double* d_out = nullptr;                              // SVec edge-indexed (tile path)
    int BI = 1, JB = 32, n_iband = 1, n_jblock = 1, g = 1;
    size_t lds = 0;
};

// CEMP.m:44-103: samples, S0Mat and the initial SVec.  need_poe: also build d_poe whenever some edge has no cycle (MPLS reads it on both
// paths); DESC_ERR_TOO_LARGE when m_pos * nsample reaches 2^31.  nsample <= 0: the rule of linprog_sij.m:43 (st.nsample says what it gave).
int cemp_build(const desc_device_problem* dp, int32_t nsample, uint64_t seed, bool need_poe, CempState& st);
// CEMP.m:107-128: max_iter rounds, beta[it] padded with its last entry; verbose: the reference's per-round line (:127)
int cemp_rounds(const desc_device_problem* dp, CempState& st, const double* beta, int32_t n_beta, int32_t max_iter, bool verbose);
// SVec edge-indexed on the device (stream-ordered behind the rounds)
const double* cemp_svec(CempState& st);
// MPLS.m:223-240 for the edges with cycles: the round with the residuals as gathered values (res_full: CSR-aligned on the tile path,
// res: edge-indexed) and the fused epilogue rh[e] = (1 - alpha) res[e] + alpha h_e
void cemp_hstep(const desc_device_problem* dp, CempState& st, const double* res_full, const double* res, double* rh, double beta, double alpha);

}  // namespace desc

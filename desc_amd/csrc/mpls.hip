// MPLS (Algorithms/MPLS.m:31-257): CEMP -> CEMP+MST initialisation -> cycle-reweighted Lie-algebraic averaging.
//   :65-158   CEMP, the text of CEMP.m:36-132: cemp.hip's two steps, whose samples and S0Mat stay resident for the loop
//   :160-193  minimum spanning tree and rotations along it: mst.hip
//   :196-216  Q = R2Q(R_init), QQ = R2Q(RijMat'), weights min(1/SVec^0.75, 1e4): the averaging core's set-up (laa.h, laa.hip)
//   :218-249  per iteration: Weighted_LAA (laa.hip); residuals (k_mpls_res); the H step -- CEMP's round on the residuals with
//             the kept S0Mat, epilogue RH = (1 - alpha) Res + alpha H fused (cemp.hip, k_cemp_round*<true>); quantile and weights
// Edges without a 3-cycle keep the reference's quirk: :239 (HVec(~IndPosbin) = 1) is commented out, their cycle product is the zero
// matrix (Rki0 / Rjk0 stay zero, :109-114), so S0 = |acos(-1/2)|/pi = 2/3, both residual terms 0, every weight 1/nsample: H = 2/3 up
// to round-off.  k_mpls_res writes their RH; the H step writes the others.
#include <algorithm>
#include <cmath>
#include <vector>

#include "cemp_state.h"
#include "laa.h"

namespace desc {
namespace {

// MPLS.m:221-222 (E = A*W(2:end,2:4) - B with W after the exp map, as k_rsvec): Res edge-indexed and, on the tile path, CSR-aligned
// (both endpoint rows) for the H step's gathers; RH of the edges without cycles (:240 with H = sum (1/nsample) 2/3)
__global__ __launch_bounds__(256) void k_mpls_res(const double* Wv, const double* B, const int32_t* ii, const int32_t* jj, int64_t m, double* res,
                                                  double* res_full, const int32_t* slot_a, const int32_t* slot_b, const int32_t* poe, double* rh,
                                                  double alpha, int nsample) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256) {
        const double r = sqrt(edge_residual_sq(Wv, B, ii, jj, e)) / M_PI;
        res[e] = r;
        if (res_full) { res_full[slot_a[e]] = r; res_full[slot_b[e]] = r; }
        if (poe && poe[e] < 0) {
            const double s0 = fabs(acos((0.0 - 1.0) / 2.0)) / M_PI, w = 1.0 / (double)nsample;      // :130 on a zero cycle matrix
            double h = 0.0;
            for (int t = 0; t < nsample; ++t) h += w * s0;                                           // :236-237
            rh[e] = (1.0 - alpha) * r + alpha * h;
        }
    }
}

// :37-63: a parameter vector shorter than the loop repeats its last entry
double padded(const double* v, int32_t len, int idx) { return v[idx < len ? idx : len - 1]; }

}  // namespace
}  // namespace desc

using namespace desc;

extern "C" int desc_mpls_run(const desc_problem* prob, const desc_mpls_params* params, int32_t device, double* R_est, double* R_init,
                             double* s_vec_out, desc_mpls_info* info) {
    if (!prob || !params || !R_est) return fail(DESC_ERR_INVALID, "NULL argument");
    auto t0 = std::chrono::steady_clock::now();
    const int rc = with_uploaded(prob, device, [&](const desc_device_problem* dp) { return desc_mpls_run_dev(dp, params, R_est, R_init, s_vec_out, info); });
    if (!rc && info) info->ms_total = ms_since(t0);
    return rc;
}

extern "C" int desc_mpls_run_dev(const desc_device_problem* dp, const desc_mpls_params* P, double* R_est, double* R_init,
                                 double* s_vec_out, desc_mpls_info* info) {
    return no_throw("desc_mpls_run_dev", [&]() -> int {
    if (!dp || !P || !R_est) return fail(DESC_ERR_INVALID, "NULL argument");
    if (!P->cemp_beta || P->n_cemp_beta < 1 || P->cemp_max_iter < 0 || P->nsample < 1)
        return fail(DESC_ERR_INVALID, "CEMP parameters: need reweighting (>= 1 entry), max_iter >= 0, nsample >= 1");
    if (!P->beta || !P->tau || !P->alpha || P->n_beta < 1 || P->n_tau < 1 || P->n_alpha < 1)
        return fail(DESC_ERR_INVALID, "MPLS parameters: reweighting, thresholding and cycle_info_ratio need >= 1 entry each");
    const int64_t n = dp->n, m = dp->m;
    if (n < 1 || m < 1) return fail(DESC_ERR_INVALID, "empty graph");
    int rc = DESC_OK;
    const bool verbose = P->verbose != 0;
    auto say = [&](const char* line) { if (verbose) printf("%s\n", line); };
    DESC_HIP(hipSetDevice(dp->device));
    auto t0 = std::chrono::steady_clock::now();
    // ---- CEMP (:65-158)
    say("sampling 3-cycles");                                                                       // :74
    CempState cs;
    if ((rc = cemp_build(dp, P->nsample, P->seed, true, cs))) return rc;
    say("Sampling Finished!"); say("Initializing"); say("Initialization completed!"); say("Reweighting Procedure Started ...");   // :96-134
    if ((rc = cemp_rounds(dp, cs, P->cemp_beta, P->n_cemp_beta, P->cemp_max_iter, verbose))) return rc;
    const double* d_svec = cemp_svec(cs);
    DESC_HIP(hipDeviceSynchronize());
    const double ms_cemp = ms_since(t0);
    say("Completed!");                                                                              // :158
    if (s_vec_out) DESC_HIP(hipMemcpy(s_vec_out, d_svec, sizeof(double) * m, hipMemcpyDeviceToHost));
    // ---- minimum spanning tree and rotations along it (:160-193)
    say("Building minimum spanning tree ...");                                                      // :161
    auto t1 = std::chrono::steady_clock::now();
    hvec<double> r_init((size_t)9 * n);
    if ((rc = mst_device(dp, d_svec, r_init.data(), nullptr))) return rc;
    const double ms_mst = ms_since(t1);
    if (R_init) std::copy(r_init.begin(), r_init.end(), R_init);
    // ---- MPLS loop (:196-249)
    auto t2 = std::chrono::steady_clock::now();
    LaaSolver L;
    if ((rc = laa_setup(dp, r_init.data(), L))) return rc;                                          // :200-206
    laa_weights(L, d_svec, INFINITY);                                                               // :210-213: clipped, not truncated
    double *d_res, *d_rh, *d_res_full = nullptr;
    if ((rc = L.alloc(&d_res, m)) || (rc = L.alloc(&d_rh, m)) || (cs.tiles && (rc = L.alloc(&d_res_full, 2 * m)))) return rc;
    say("Rotation Initialized!"); say("Start MPLS reweighting ...");                                // :215-216
    const double stop_threshold = P->stop_threshold;
    const int max_iter = P->max_iter;
    double score = INFINITY;
    int Iteration = 1;
    while (score > stop_threshold && Iteration < max_iter) {                                        // :218
        const double beta = padded(P->beta, P->n_beta, Iteration - 1), tau = padded(P->tau, P->n_tau, Iteration - 1),
                     alpha = padded(P->alpha, P->n_alpha, Iteration - 1);
        if ((rc = laa_step(L, &score))) return rc;                                                  // :220
        hipLaunchKernelGGL(k_mpls_res, dim3(L.egrid), dim3(256), 0, 0, L.d_Wv, L.d_B, dp->d_ii, dp->d_jj, m, d_res, d_res_full, cs.d_slot_a, cs.d_slot_b,
                           cs.d_poe, d_rh, alpha, (int)cs.nsample);                                 // :221-222 (+ :240 without cycles)
        cemp_hstep(dp, cs, d_res_full, d_res, d_rh, beta, alpha);                                   // :223-240
        double thresh = 0.0;
        if ((rc = laa_quantile(L, d_rh, tau, &thresh))) return rc;                                  // :243
        laa_weights(L, d_rh, thresh);                                                               // :241-245
        DESC_HIP(hipGetLastError());
        if (verbose) printf("Iter %d: ||\xce\x94R||= %f\n", Iteration, score);                      // :247
        ++Iteration;
    }
    if ((rc = laa_finish(L, Iteration - 1, R_est))) return rc;                                      // :251-254
    say("DONE!");
    if (verbose) fflush(stdout);
    if (info) {
        info->iters = Iteration - 1; info->cg_iters = L.cg.total; info->cg_unconverged = L.cg.unconverged; info->reserved = 0;
        info->m_pos = cs.mp; info->score = score; info->cg_residual = L.cg.worst;
        info->ms_cemp = ms_cemp; info->ms_mst = ms_mst; info->ms_loop = ms_since(t2); info->ms_total = ms_since(t0);
    }
    return DESC_OK;
    });
}

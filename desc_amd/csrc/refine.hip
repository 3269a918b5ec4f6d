// DESC refinement tail: reweighted Lie-algebraic averaging.
//
// Reference text reproduced:
//   Algorithms/DESC.m:265-313      RR = R_ij', Q = R2Q(R_init), QQ = R2Q(RR); weights 1/S^0.75 clipped to
//                                  [1e-4, 1e4]; loop: Weighted_LAA, residuals, RSVec = (1-lam) Res + lam S,
//                                  quantile truncation, stop at score <= 1e-3 or 100 iterations; q2R
// Weighted_LAA, the quantile and the weights are the shared core (laa.h, laa.hip); this file is the loop around them.
#include <algorithm>
#include <cmath>

#include "laa.h"

namespace desc {
namespace {

// DESC.m:289-291: E = A*W(2:end,2:4) - B, ResVec = |E|/pi, RSVec = (1-lam) ResVec + lam S
__global__ void k_rsvec(const double* Wv, const double* B, const int32_t* ii, const int32_t* jj, const double* S, double* RS,
                        int64_t m, double lam) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x)
        RS[e] = rsvec_value(Wv, B, ii, jj, S, e, lam);
}

}  // namespace
}  // namespace desc

using namespace desc;

extern "C" int desc_refine_run(const desc_problem* prob, const double* s_vec, const double* R_init, double stop_threshold,
                               int32_t max_iters, int32_t device, double* R_out, desc_refine_info* info) {
    if (!prob || !s_vec || !R_init || !R_out) return fail(DESC_ERR_INVALID, "NULL argument");
    if (prob->n == 0) return validate_problem(prob, true);
    auto t0 = std::chrono::steady_clock::now();
    const int rc = with_uploaded(prob, device, [&](const desc_device_problem* dp) { return desc_refine_run_dev(dp, s_vec, R_init, stop_threshold, max_iters, R_out, info); });
    if (!rc && info) info->ms_total = ms_since(t0);
    return rc;
}

extern "C" int desc_refine_run_dev(const desc_device_problem* dp, const double* s_vec, const double* R_init, double stop_threshold,
                                   int32_t max_iters, double* R_out, desc_refine_info* info) {
    return no_throw("desc_refine_run_dev", [&]() -> int {
    if (!dp || !s_vec || !R_init || !R_out) return fail(DESC_ERR_INVALID, "NULL argument");
    int rc = DESC_OK;
    const int64_t n = dp->n, m = dp->m;
    if (n == 0) return DESC_OK;
    DESC_HIP(hipSetDevice(dp->device));
    auto t0 = std::chrono::steady_clock::now();
    if (stop_threshold <= 0) stop_threshold = 1e-3;      // DESC.m:272
    if (max_iters <= 0) max_iters = 100;

    // initial weights (DESC.m:274-282): quantile(S_vec, 1) = max -> nothing is truncated yet; evaluated on
    // the device by the same kernel as the re-weighting steps
    double thresh0 = -INFINITY;
    for (int64_t e = 0; e < m; ++e) thresh0 = std::max(thresh0, s_vec[e]);
    LaaSolver L;
    if ((rc = laa_setup(dp, R_init, L))) return rc;
    double *d_S, *d_RS;
    if ((rc = L.alloc(&d_S, m)) || (rc = L.alloc(&d_RS, m))) return rc;
    if (m) DESC_HIP(hipMemcpy(d_S, s_vec, sizeof(double) * m, hipMemcpyHostToDevice));
    laa_weights(L, d_S, thresh0);

    double score = INFINITY, quant_ratio = 1.0;
    const double quant_ratio_min = 0.8;
    int Iteration = 1;
    while (score > stop_threshold && Iteration < max_iters) {                               // DESC.m:287
        const double lam = 1.0 / (Iteration + 1);
        if ((rc = laa_step(L, &score))) return rc;                                          // Weighted_LAA
        // ---- residuals and new weights (DESC.m:289-303)
        if (m) {
            hipLaunchKernelGGL(k_rsvec, dim3(L.egrid), dim3(256), 0, 0, L.d_Wv, L.d_B, dp->d_ii, dp->d_jj, d_S, d_RS, m, lam);
            quant_ratio = std::max(quant_ratio_min, quant_ratio - 0.05);
            double thresh = 0.0;                                                            // quantile(RSVec, quant_ratio)  (DESC.m:299)
            if ((rc = laa_quantile(L, d_RS, quant_ratio, &thresh))) return rc;
            laa_weights(L, d_RS, thresh);
        }
        DESC_HIP(hipGetLastError());
        if (info && info->verbose) printf("Iter %d: ||\xce\x94R||= %f\n", Iteration, score);                 // DESC.m:305
        ++Iteration;
    }
    if ((rc = laa_finish(L, Iteration - 1, R_out))) return rc;
    if (info) {
        info->iters = Iteration - 1; info->score = score; info->cg_iters = L.cg.total;
        info->cg_unconverged = L.cg.unconverged; info->cg_residual = L.cg.worst;
        info->ms_total = ms_since(t0);
    }
    return DESC_OK;
    });
}

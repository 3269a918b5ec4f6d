// Internal: the Lie-algebraic averaging core on a device problem -- the reweighted step of Utils/Weighted_LAA.m, the Jacobi-PCG on the
// grounded graph Laplacian under it, the quantile and the quaternion maps.  Implemented in laa.hip; used by the DESC refinement tail
// (Algorithms/DESC.m:265-313, refine.hip), MPLS (Algorithms/MPLS.m:196-254, mpls.hip) and IRLS_GM / IRLS_L12 (irls.hip).
#pragma once
#include "device_utils.h"
#include "laa_math.h"

namespace desc {

// the PCG's device-resident scalars, per coordinate; bad: the coordinate broke down (only set when breakdowns are tracked)
struct CgScal { double rz[3], rz_new[3], pq[3], bnorm[3], rnorm[3]; int bad[3], pad; };
// PCG bookkeeping over the solves of one loop: steps (each solve's true count rounded up to its probe interval), solves that stopped at
// the iteration cap, the largest relative residual |r| / |b| a solve ended with
struct CgCount { int total = 0, unconverged = 0; double worst = 0.0; };

// Device state of one refinement loop: rotations as quaternions, the relative rotations' quaternions, the edge weights,
// the PCG work arrays and the quantile scratch.  laa_setup allocates and fills it; the buffers live until destruction.
struct LaaSolver : DevArena {
    const desc_device_problem* dp = nullptr;
    int64_t n = 0, m = 0;
    int egrid = 1, ngrid = 1, rgrid = 1, sgrid = 64;
    int8_t* d_sgn = nullptr;
    double *d_Rinit = nullptr, *d_w = nullptr, *d_B = nullptr, *d_rhs = nullptr, *d_diag = nullptr, *d_x = nullptr, *d_r = nullptr,
           *d_z = nullptr, *d_p = nullptr, *d_q = nullptr, *d_Wv = nullptr, *d_score = nullptr, *d_Rout = nullptr;
    Quat *d_Q = nullptr, *d_QQ = nullptr;
    CgScal* d_sc = nullptr;
    double *d_mm = nullptr, *d_cand = nullptr;
    unsigned* d_qh = nullptr;
    CgCount cg;                               // of laa_step's solves
    hvec<double> part;
};

// allocate, upload R_init (n*9 host doubles, 3x3xn column-major), Q = R2Q(R_init), QQ = R2Q(permute(RijMat, [2,1,3]))
int laa_setup(const desc_device_problem* dp, const double* R_init, LaaSolver& L);
// Weighted_LAA.m:4-51 with the weights in L.d_w: edge log map B, normal equations by PCG, Q <- Q * exp(W); *score = :40
int laa_step(LaaSolver& L, double* score);
// Jacobi-PCG for the three systems A' diag(w_c) A x_c = rhs_c (A: incidence matrix with node 0 grounded) in L's work arrays: scalars
// on the device, the host probes |r| <= 1e-13 |b| every `probe` steps over the coordinates in act; x, rhs, diag are n x 3 / n device
// arrays of the caller.
//   W3     the operator weight of edge e, coordinate c is w[3 e + c] and the Jacobi diagonal diag[3 v + c] (the primal-dual Newton
//          systems); else w[e] * w[e] for all three and diag[v] (Weighted_LAA's normal equations)
//   TRACK  a breakdown (a non-finite p'Hp or r'z, or p'Hp <= 0 while r'z > 0) freezes its coordinate (alpha = 0 from then on), takes it
//          out of the convergence test and is returned in bad[c]; else bad[] comes back 0.  Off for laa_step, and to stay off: with
//          it a degenerate input would return something else.
template <bool W3, bool TRACK>
int laa_pcg(LaaSolver& L, const double* w, const double* rhs, const double* diag, double* x, const int act[3], int probe, CgCount& count, int bad[3]);
// QQ = R2Q(blocks) of m blocks that are already in the reference's RR orientation (no transpose): replaces laa_setup's
// R2Q(permute(RijMat, [2,1,3])) when the edge rotations were modified first (IRLS_GM.m:82-93, irls.hip)
void laa_set_qq(LaaSolver& L, const double* d_blocks);
// Weighted_LAA.m:9-35 alone: the edge log map of the current Q into L.d_B (BoxMedianSO3Graph.m:143-160 is the same text)
void laa_edge_log(LaaSolver& L);
// weights from a per-edge residual vector (DESC.m:298-303, MPLS.m:241-245): w = min(1/x^0.75, 1e4), 1e-4 where x > thresh
void laa_weights(LaaSolver& L, const double* d_x, double thresh);
// MATLAB quantile(x, p) of a device vector of m entries
int laa_quantile(LaaSolver& L, const double* d_x, double p, double* result);
// q2R.m of every node into R_out (n*9 host doubles); prints the reference's warning when a PCG solve stopped at its cap
int laa_finish(LaaSolver& L, int iterations, double* R_out);

// ---- copies of the test hooks (desc_test_laa_* in laa.hip, desc_test_irls_* in irls.hip): `count` host elements into a fresh block of
// the arena; `count` elements back after the device has drained, with the launch errors it left
template <class T>
int hook_upload(DevArena& A, const T* host, int64_t count, T** out) {
    int rc = A.alloc(out, (size_t)count);
    if (rc) return rc;
    if (count) DESC_HIP(hipMemcpy(*out, host, sizeof(T) * count, hipMemcpyHostToDevice));
    return DESC_OK;
}
// the solver state of laa_setup on dp with identity R_init, for the hooks: grids, incidence signs, work arrays (laa.hip)
int hook_solver(const desc_device_problem* dp, LaaSolver& L);
template <class T>
int hook_download(T* host, const T* dev, int64_t count) {
    DESC_HIP(hipDeviceSynchronize());
    DESC_HIP(hipGetLastError());
    if (count) DESC_HIP(hipMemcpy(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost));
    return DESC_OK;
}

}  // namespace desc

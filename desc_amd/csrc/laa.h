// Internal: the reweighted Lie-algebraic averaging step (Utils/Weighted_LAA.m) on a device problem, shared by the DESC
// refinement tail (Algorithms/DESC.m:265-313) and MPLS (Algorithms/MPLS.m:196-254).  Kernels and driver in refine.hip.
#pragma once
#include "common.h"

namespace desc {

struct Quat { double a, x, y, z; };

// Device state of one refinement loop: rotations as quaternions, the relative rotations' quaternions, the edge weights,
// the PCG work arrays and the quantile scratch.  laa_setup allocates and fills it; the buffers live until destruction.
struct LaaSolver {
    hvec<void*> blocks;
    const desc_device_problem* dp = nullptr;
    int64_t n = 0, m = 0;
    int egrid = 1, ngrid = 1, rgrid = 1, sgrid = 64;
    int8_t* d_sgn = nullptr;
    double *d_Rinit = nullptr, *d_w = nullptr, *d_B = nullptr, *d_rhs = nullptr, *d_diag = nullptr, *d_x = nullptr, *d_r = nullptr,
           *d_z = nullptr, *d_p = nullptr, *d_q = nullptr, *d_Wv = nullptr, *d_score = nullptr, *d_Rout = nullptr;
    Quat *d_Q = nullptr, *d_QQ = nullptr;
    void* d_sc = nullptr;                     // CG scalars (device-resident)
    double *d_mm = nullptr, *d_cand = nullptr;
    unsigned* d_qh = nullptr;
    int cg_total = 0, cg_unconverged = 0;
    double cg_worst = 0.0;
    hvec<double> part;
    ~LaaSolver();
    template <class T> int alloc(T** out, size_t count);
};

// allocate, upload R_init (n*9 host doubles, 3x3xn column-major), Q = R2Q(R_init), QQ = R2Q(permute(RijMat, [2,1,3]))
int laa_setup(const desc_device_problem* dp, const double* R_init, LaaSolver& L);
// Weighted_LAA.m:4-51 with the weights in L.d_w: edge log map B, normal equations by PCG, Q <- Q * exp(W); *score = :40
int laa_step(LaaSolver& L, double* score);
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

}  // namespace desc

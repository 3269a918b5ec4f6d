// What the kernels that produce 3x3 blocks one thread per block share: the projection onto SO(3) by the per-thread Jacobi SVD, and the
// store of a workgroup's blocks through LDS.  Shared by models_batch.hip (the generator's node and edge passes) and align_batch.hip
// (R_align of Rotation_Alignment.m:24-25): one text, so a block gets the same bits whichever of them projects it.
#pragma once
#include "irls_math.h"

namespace desc {

// P(Q) = U diag(1, 1, det(U V')) V' of the column-major block q (destroyed), by the one-sided Jacobi SVD of irls_math.h.  The third
// left vector does not need sigma_3: det(U) u3 = u1 x u2, so P = u1 v1' + u2 v2' + det(V) (u1 x u2) v3' (as small_dense.h::project_so3).
__device__ inline void mb_project(double* q, double* R) {
    double v[9], s[3];
    svd3(q, v, s);
    double u1[3], u2[3], u3[3];
    double n1 = 0, n2 = 0, d12 = 0;
    for (int r = 0; r < 3; ++r) n1 += q[r] * q[r];
    n1 = sqrt(n1);
    for (int r = 0; r < 3; ++r) u1[r] = q[r] / n1;
    for (int r = 0; r < 3; ++r) d12 += u1[r] * q[3 + r];
    for (int r = 0; r < 3; ++r) { u2[r] = q[3 + r] - d12 * u1[r]; n2 += u2[r] * u2[r]; }
    n2 = sqrt(n2);
    for (int r = 0; r < 3; ++r) u2[r] = u2[r] / n2;
    const double dv = v[0] * (v[4] * v[8] - v[7] * v[5]) - v[3] * (v[1] * v[8] - v[7] * v[2]) + v[6] * (v[1] * v[5] - v[4] * v[2]);
    const double sg = dv < 0 ? -1.0 : 1.0;
    u3[0] = sg * (u1[1] * u2[2] - u1[2] * u2[1]);
    u3[1] = sg * (u1[2] * u2[0] - u1[0] * u2[2]);
    u3[2] = sg * (u1[0] * u2[1] - u1[1] * u2[0]);
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) R[r + 3 * c] = (u1[r] * v[c] + u2[r] * v[3 + c]) + u3[r] * v[6 + c];
}

// The workgroup's 256 blocks (thread t holds item first + t) to dst + 9 * first: through LDS, consecutive lanes write consecutive
// doubles.  Called by all 256 threads; nvalid: the items of this workgroup that exist.
__device__ __forceinline__ void mb_store_blocks(double* lds, double* dst, const double* blk, int nvalid) {
    __syncthreads();                                              // the staging area's last readers are done
    for (int k = 0; k < 9; ++k) lds[9 * (int)threadIdx.x + k] = blk[k];
    __syncthreads();
    for (int t = (int)threadIdx.x; t < 9 * nvalid; t += 256) dst[t] = lds[t];
}

}  // namespace desc

// The arithmetic of CEMP (Algorithms/CEMP.m:70-128) that the single-problem kernels (cemp.hip) and the batched ones (cemp_batch.hip)
// share: one text, so an edge gets the same bits whichever of them computes it (as pgd_math.h and small_dense.h for their callers).
//   cemp_cycle_dist   :70-100  d_ijk = |acos((tr(Rij Rjk Rki) - 1) / 2)| / pi of one sampled cycle
//   cemp_edge_round   :107-128 one round of one edge: w = exp(-beta (s_ik + s_jk)), normalised over the edge's samples, s_ij = sum w .* S0
// Both are called by a whole wave for one edge: sample s sits on lane s & 63, sums over lanes are group_sum<64>'s fixed butterfly.
#pragma once
#include <cmath>

#include "device_utils.h"

namespace desc {

__device__ __forceinline__ double abs_acos_ext_c(double x) {
    if (x > 1.0) return acosh(x);
    if (x < -1.0) return hypot(M_PI, acosh(-x));
    return acos(x);
}

// A = R_ij, pb = the stored block of edge {j,k}, pc = that of {k,i}; tb / tc: the stored block is the transpose of the factor
// (orientation matters only for fetching R_jk / R_ki, CEMP.m:75-76)
__device__ __forceinline__ double cemp_cycle_dist(const double* A, const double* pb, const double* pc, bool tb, bool tc) {
    double tr = 0.0;
    for (int r = 0; r < 3; ++r) {
        double P[3];
        for (int q = 0; q < 3; ++q) {
            double a2 = 0.0;
            for (int u = 0; u < 3; ++u) a2 = a2 + A[r + 3 * u] * (tb ? pb[q + 3 * u] : pb[u + 3 * q]);
            P[q] = a2;
        }
        double a3 = 0.0;
        for (int u = 0; u < 3; ++u) a3 = a3 + P[u] * (tc ? pc[r + 3 * u] : pc[u + 3 * r]);
        tr = tr + a3;
    }
    return abs_acos_ext_c((tr - 1.0) / 2.0) / M_PI;
}

// The new s_ij of the edge whose nsample slots start at l * nsample (every lane returns it).  e_jk / e_ki index S_old.  Three classes of
// nsample: <= 64 and <= 256 keep the weights in registers and divide once per edge (the reference divides every weight: the same to
// 1 ulp), longer samples make two passes and divide every weight by the sum.
__device__ __forceinline__ double cemp_edge_round(int64_t l, int lane, int nsample, double beta, const int32_t* e_jk, const int32_t* e_ki,
                                                  const double* S0, const double* S_old) {
    if (nsample <= 4 * 64) {                       // weights stay in registers: one pass over the samples
        double wr[4] = {0.0, 0.0, 0.0, 0.0}, dr[4] = {0.0, 0.0, 0.0, 0.0};
        double wsum = 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int s = lane + 64 * u;
            if (s < nsample) {
                const int64_t c = l * nsample + s;
                wr[u] = exp(-beta * (S_old[e_ki[c]] + S_old[e_jk[c]]));      // :118-120
                dr[u] = S0[c];
                wsum += wr[u];
            }
        }
        wsum = group_sum<64>(wsum);
        double acc = 0.0;
        const double rws = 1.0 / wsum;                 // one division per edge (the reference divides every weight: the same to 1 ulp)
#pragma unroll
        for (int u = 0; u < 4; ++u) if (lane + 64 * u < nsample) acc += (wr[u] * rws) * dr[u];   // :122-125
        return group_sum<64>(acc);
    }
    double wsum = 0.0;
    for (int s = lane; s < nsample; s += 64) {
        const int64_t c = l * nsample + s;
        wsum += exp(-beta * (S_old[e_ki[c]] + S_old[e_jk[c]]));                  // :118-120
    }
    wsum = group_sum<64>(wsum);
    double acc = 0.0;
    for (int s = lane; s < nsample; s += 64) {
        const int64_t c = l * nsample + s;
        const double w = exp(-beta * (S_old[e_ki[c]] + S_old[e_jk[c]]));
        acc += (w / wsum) * S0[c];                                               // :122-125
    }
    return group_sum<64>(acc);
}

}  // namespace desc

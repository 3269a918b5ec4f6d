// The per-element arithmetic of the Lie-algebraic averaging core (Utils/Weighted_LAA.m, Build_Amatrix.m, R2Q.m, q2R.m, DESC.m:289-303),
// shared by the kernels of the single path (laa.hip, refine.hip, mpls.hip, irls.hip) and the batched refinement (refine_batch.hip): the
// same text on both paths is what makes desc_refine_batch_run's result the single call's bit for bit.
//
// The library is built without contraction and fast-math: an expression tree kept as it is gives the same bits, so operand order and
// bracketing below are part of the interface.
#pragma once
#include <cmath>

#include "device_utils.h"

namespace desc {

struct Quat { double a, x, y, z; };

// Hamilton product a * b.  inv(q) * b as the reference writes it (the negated product, the same rotation) is qmul({-q.a, q.x, q.y, q.z}, b).
__host__ __device__ __forceinline__ Quat qmul(const Quat& a, const Quat& b) {
    Quat o;
    o.a = a.a * b.a - (a.x * b.x + a.y * b.y + a.z * b.z);
    o.x = a.a * b.x + b.a * a.x + (a.y * b.z - a.z * b.y);
    o.y = a.a * b.y + b.a * a.y + (a.z * b.x - a.x * b.z);
    o.z = a.a * b.z + b.a * a.z + (a.x * b.y - a.y * b.x);
    return o;
}
// exp map of the tangent vector t (Weighted_LAA.m:42-46, BoxMedianSO3Graph.m:176-180): *theta = |t|; NaN -> 0 (theta = 0 gives the zero
// quaternion part, as the reference)
__device__ __forceinline__ Quat qexp(double t1, double t2, double t3, double* theta) {
    const double th = sqrt(t1 * t1 + t2 * t2 + t3 * t3);
    Quat w;
    w.a = cos(th / 2.0);
    const double f = sin(th / 2.0) / th;
    w.x = t1 * f; w.y = t2 * f; w.z = t3 * f;
    if (isnan(w.a)) w.a = 0.0;
    if (isnan(w.x)) w.x = 0.0;
    if (isnan(w.y)) w.y = 0.0;
    if (isnan(w.z)) w.z = 0.0;
    *theta = th;
    return w;
}
// |(A x - B)_e|^2 of edge e = (i, j): sum over the coordinates of ((x_j - x_i)_c - B_e,c)^2, node 0 grounded (its x counts as 0)
__device__ __forceinline__ double edge_residual_sq(const double* x, const double* B, const int32_t* ii, const int32_t* jj, int64_t e) {
    const int i = ii[e], j = jj[e];
    double s = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double ax = (j > 0 ? x[3 * j + c] : 0.0) - (i > 0 ? x[3 * i + c] : 0.0);
        const double d = ax - B[3 * e + c];
        s += d * d;
    }
    return s;
}

// R2Q.m:9-12 for a column-major 3x3 block (optionally transposed)
__device__ __forceinline__ Quat r2q(const double* R, bool transpose) {
    const double r11 = R[0], r22 = R[4], r33 = R[8];
    double r32 = R[5], r23 = R[7], r13 = R[6], r31 = R[2], r21 = R[1], r12 = R[3];      // (r,c) at r + 3c
    if (transpose) { double t; t = r32; r32 = r23; r23 = t; t = r13; r13 = r31; r31 = t; t = r21; r21 = r12; r12 = t; }
    Quat q;
    q.a = (r11 + r22 + r33 - 1.0) / 2.0; q.x = (r32 - r23) / 2.0; q.y = (r13 - r31) / 2.0; q.z = (r21 - r12) / 2.0;
    q.a = sqrt((q.a + 1.0) / 2.0);
    q.x = (q.x / q.a) / 2.0; q.y = (q.y / q.a) / 2.0; q.z = (q.z / q.a) / 2.0;
    return q;
}
// q2R.m: the column-major 3x3 block of q into M[9]
__device__ __forceinline__ void q2r(const Quat& q, double* M) {
    M[0] = 1; M[1] = 0; M[2] = 0; M[3] = 0; M[4] = 1; M[5] = 0; M[6] = 0; M[7] = 0; M[8] = 1;
    const double c2 = q.a;
    if (fabs(fabs(c2) - 1.0) > 1e-12) {
        const double s2 = sqrt(q.x * q.x + q.y * q.y + q.z * q.z);
        const double s = 2.0 * s2 * c2, c = 2.0 * c2 * c2 - 1.0, cc = 1.0 - c;
        const double n1 = q.x / s2, n2 = q.y / s2, n3 = q.z / s2;
        const double n12 = n1 * n2 * cc, n23 = n2 * n3 * cc, n31 = n3 * n1 * cc, n1s = n1 * s, n2s = n2 * s, n3s = n3 * s;
        M[0] = c + n1 * n1 * cc; M[3] = n12 - n3s;        M[6] = n31 + n2s;        // column-major: (r,c) at r + 3c
        M[1] = n12 + n3s;        M[4] = c + n2 * n2 * cc; M[7] = n23 - n1s;
        M[2] = n31 - n2s;        M[5] = n23 + n1s;        M[8] = c + n3 * n3 * cc;
    }
}

// Weighted_LAA.m:9-37: residual quaternion w = -(conj(Qj) (QQ Qi)), b = its log map (NaN -> 0, :35)
__device__ __forceinline__ void edge_log(const Quat& qq, const Quat& qi, const Quat& qj, double* b) {
    const Quat w = qmul(qq, qi);
    const Quat v = qmul(Quat{-qj.a, qj.x, qj.y, qj.z}, w);                       // inv(Qj) * w as written in the reference
    const double s2 = sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
    double v1 = 2.0 * atan2(s2, v.a);
    if (v1 < -M_PI) v1 += 2.0 * M_PI;
    if (v1 >= M_PI) v1 -= 2.0 * M_PI;
    const double f = v1 / s2;
    double b1 = v.x * f, b2 = v.y * f, b3 = v.z * f;
    if (isnan(b1)) b1 = 0.0;                                                     // :35
    if (isnan(b2)) b2 = 0.0;
    if (isnan(b3)) b3 = 0.0;
    b[0] = b1; b[1] = b2; b[2] = b3;
}

// Row sums over the CSR slots [t0, t1) of one node, taken by the 16 lanes of a DPP row: lane l16 adds the slots t0 + l16, + 16, ... in
// order, group16_sum combines the lanes; every lane returns the row's totals.  All 16 lanes of the row must call (an idle row passes
// t0 = t1), and the lanes of a wave must arrive together.
// the right-hand side and the diagonal of the normal equations A'W^2A x = A'W^2 B: a[c] = sum_t sgn * w_e^2 * B_e,c ; dg = sum_t w_e^2
__device__ __forceinline__ void rhs_row16(const int32_t* eid, const int8_t* sgn, const double* wts, const double* B, int t0, int t1, int l16,
                                          double* a, double* dg_out) {
    double a0 = 0, a1 = 0, a2 = 0, dg = 0;
    for (int t = t0 + l16; t < t1; t += 16) {
        const int e = eid[t];
        const double w2 = wts[e] * wts[e], sg = (double)sgn[t];
        a0 += sg * w2 * B[3 * (int64_t)e]; a1 += sg * w2 * B[3 * (int64_t)e + 1]; a2 += sg * w2 * B[3 * (int64_t)e + 2];
        dg += w2;
    }
    a[0] = group16_sum(a0); a[1] = group16_sum(a1); a[2] = group16_sum(a2); *dg_out = group16_sum(dg);
}
// the grounded graph Laplacian: a[c] = sum_t w_e,c (p_v - p_u); W3: the weight of edge e, coordinate c is w[3 e + c], else w[e] * w[e]
template <bool W3>
__device__ __forceinline__ void lap_row16(const int32_t* adj, const int32_t* eid, const double* w, const double* p, int v, int t0, int t1, int l16,
                                          double* a) {
    double a0 = 0, a1 = 0, a2 = 0;
    if (t0 < t1) {
        const double p0 = p[3 * v], p1 = p[3 * v + 1], p2 = p[3 * v + 2];
        for (int t = t0 + l16; t < t1; t += 16) {
            const int u = adj[t];
            const int64_t e = eid[t];
            const double w0 = W3 ? w[3 * e] : w[e] * w[e], w1 = W3 ? w[3 * e + 1] : w0, w2 = W3 ? w[3 * e + 2] : w0;
            a0 += w0 * (p0 - p[3 * u]); a1 += w1 * (p1 - p[3 * u + 1]); a2 += w2 * (p2 - p[3 * u + 2]);
        }
    }
    a[0] = group16_sum(a0); a[1] = group16_sum(a1); a[2] = group16_sum(a2);
}

// z = r / diag (0 at the grounded node and where the diagonal is not positive)
template <bool W3>
__device__ __forceinline__ double jacobi(const double* diag, int v, int c, double rv) {
    const double d = diag[W3 ? 3 * v + c : v];
    return (v > 0 && d > 0) ? rv / d : 0.0;
}
// the PCG's step lengths from its scalars: alpha = r'z / p'Hp (0 unless p'Hp > 0), beta = r'z_new / r'z (0 unless r'z > 0)
__device__ __forceinline__ double cg_alpha(double rz, double pq) { return pq > 0 ? rz / pq : 0.0; }
__device__ __forceinline__ double cg_beta(double rz, double rz_new) { return rz > 0 ? rz_new / rz : 0.0; }
// a breakdown of the PCG (tracked only for the primal-dual Newton systems): a non-finite p'Hp or r'z, or p'Hp <= 0 while r'z > 0
__device__ __forceinline__ bool cg_breaks(double pq, double rz) { return !isfinite(pq) || !isfinite(rz) || (pq <= 0.0 && rz > 0.0); }
// the probe's test on one coordinate: not yet at |r| <= 1e-13 |b|
__host__ __device__ __forceinline__ bool cg_unfinished(double rnorm, double bnorm) { return rnorm > 1e-26 * bnorm && rnorm > 1e-300; }

// Weighted_LAA.m:40-50 for one node: W = exp map of the tangent solution x (:42-46), its vector part into wv, Q <- Q * W; returns
// theta = |x|, the node's term of the score (:40)
__device__ __forceinline__ double node_update(const double* x, Quat* q, double* wv) {
    double theta;
    const Quat w = qexp(x[0], x[1], x[2], &theta);
    wv[0] = w.x; wv[1] = w.y; wv[2] = w.z;
    *q = qmul(*q, w);
    return theta;
}
// the score's sum over one chunk of 256 rows, one row per thread of a 256-thread workgroup: the 64 lanes of a wave by the fixed
// butterfly, then the four waves through sh[4] as (sh0 + sh1) + (sh2 + sh3).  Holds a barrier; the caller places another one before sh
// is written again.
__device__ __forceinline__ double score_chunk_sum(double sc, double* sh) {
    sc = group_sum<64>(sc);                                                           // the score's order of summation: not to be moved
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = sc;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// DESC.m:289-291: E = A*W(2:end,2:4) - B, ResVec = |E|/pi, RSVec = (1-lam) ResVec + lam S
__device__ __forceinline__ double rsvec_value(const double* Wv, const double* B, const int32_t* ii, const int32_t* jj, const double* S, int64_t e, double lam) {
    return (1.0 - lam) * (sqrt(edge_residual_sq(Wv, B, ii, jj, e)) / M_PI) + lam * S[e];
}
// DESC.m:298-303, MPLS.m:241-245: w = min(1/x^0.75, wmax), wmin where x > thresh
__device__ __forceinline__ double laa_weight(double x, double thresh, double wmax, double wmin) {
    double w = 1.0 / pow(x, 0.75);
    if (w > wmax) w = wmax;
    if (x > thresh) w = wmin;
    return w;
}

// MATLAB quantile(x, p) of m > 0 values: Hazen plotting positions (k - 0.5) / m, linear interpolation, clamped.  What the caller has to
// find: HAZEN_MIN the minimum, HAZEN_MAX the maximum, HAZEN_PAIR the order statistics *k0 and *k0 + 1 (0-based ranks), joined by
// hazen_interp with *fr.
enum { HAZEN_MIN = 0, HAZEN_MAX = 1, HAZEN_PAIR = 2 };
__host__ __device__ __forceinline__ int hazen_position(int64_t m, double p, int64_t* k0, double* fr) {
    const double pos = p * (double)m + 0.5;                 // 1-based fractional index
    if (pos <= 1.0) return HAZEN_MIN;
    if (pos >= (double)m) return HAZEN_MAX;
    *k0 = (int64_t)floor(pos) - 1;                          // 0-based rank of the lower order statistic; the upper one is k0 + 1
    *fr = pos - floor(pos);
    return HAZEN_PAIR;
}
// all values equal (or none comparable): the quantile is lo, whatever the position
__host__ __device__ __forceinline__ bool hazen_flat(double lo, double hi) { return !(hi > lo); }
__host__ __device__ __forceinline__ double hazen_interp(double a, double b, double fr) { return a + fr * (b - a); }

}  // namespace desc

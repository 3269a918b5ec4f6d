// The per-element arithmetic and the scalar decisions of IRLS_GM / IRLS_L12 (Algorithms/IRLS_GM.m:82-93, Utils/BoxMedianSO3Graph.m and
// its l1decode_pd, RobustMeanSO3Graph.m:169-170, L12.m:169-171), shared by the kernels of the single path (irls.hip) and the batched one
// (irls_batch.hip): the same text on both paths is what makes desc_irls_batch_run's result the single call's bit for bit (as laa_math.h
// for the averaging core and lp_math.h for the LP).
//   irls_edge_status / irls_edge_project   the per-edge checks and P = U round(S) V'
//   pd_*_at, pd_resid_*, pd_gather_*       one element of k_pd_init / _pre / _dir / _resid / _accept / _gather
//   l1_node_update, irls_weight            one node of the L1 update, one edge of the reweighting
//   pd_* / l1_* / irls_* scalar rules      what pd_solve and the two outer loops decide between launches; __host__ __device__: the
//                                          host loop of irls.hip and the workgroup of irls_batch.hip take them from one text
//   irls_tree_sequence                     the graph part of the spanning-tree start (BoxMedianSO3Graph.m:79-114), host only
// The library is built without contraction and fast-math: operand order and bracketing below are part of the interface.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "laa_math.h"

namespace desc {

// ---- stage 3: per-edge checks and projection ---------------------------------------------------------------------------------------
// one-sided Jacobi SVD of a 3x3 column-major matrix: A V = U S; a[] ends as U S (columns), v[] as V; s sorted descending
__device__ inline void svd3(double a[9], double v[9], double s[3]) {
    for (int k = 0; k < 9; ++k) v[k] = (k % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
        for (int pr = 0; pr < 3; ++pr) {
            const int p = pr == 2 ? 1 : 0, q = pr == 0 ? 1 : 2;
            double al = 0, be = 0, ga = 0;
            for (int r = 0; r < 3; ++r) { al += a[3 * p + r] * a[3 * p + r]; be += a[3 * q + r] * a[3 * q + r]; ga += a[3 * p + r] * a[3 * q + r]; }
            if (!(fabs(ga) > 1e-300 && fabs(ga) > 1e-17 * sqrt(al * be))) continue;
            rotated = true;
            const double zeta = (be - al) / (2.0 * ga);
            const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
            for (int r = 0; r < 3; ++r) {
                const double ap = a[3 * p + r], aq = a[3 * q + r];
                a[3 * p + r] = c * ap - sn * aq; a[3 * q + r] = sn * ap + c * aq;
                const double vp = v[3 * p + r], vq = v[3 * q + r];
                v[3 * p + r] = c * vp - sn * vq; v[3 * q + r] = sn * vp + c * vq;
            }
        }
        if (!rotated) break;
    }
    for (int k = 0; k < 3; ++k) s[k] = sqrt(a[3 * k] * a[3 * k] + a[3 * k + 1] * a[3 * k + 1] + a[3 * k + 2] * a[3 * k + 2]);
    for (int i = 0; i < 2; ++i)                                               // descending, as MATLAB's svd
        for (int k = 0; k < 2 - i; ++k)
            if (s[k] < s[k + 1]) {
                double t = s[k]; s[k] = s[k + 1]; s[k + 1] = t;
                for (int r = 0; r < 3; ++r) {
                    t = a[3 * k + r]; a[3 * k + r] = a[3 * k + 3 + r]; a[3 * k + 3 + r] = t;
                    t = v[3 * k + r]; v[3 * k + r] = v[3 * k + 3 + r]; v[3 * k + 3 + r] = t;
                }
            }
}

// IRLS_GM.m:82-91 for one edge: RR = Rij' (column-major, RR orientation) into a, its determinant, its SVD (a = U S, v = V, s).
// Returns the status: 3 det <= 0, 2 all three |s - 1| >= 0.1, 1 all three >= 0.01 (warning), 0 fine.
__device__ __forceinline__ int irls_edge_status(const double* rij9, double a[9], double v[9], double s[3], double* det_out) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) a[r + 3 * c] = rij9[c + 3 * r];                  // RR(r, c) = Rij(c, r)
    const double det = a[0] * (a[4] * a[8] - a[7] * a[5]) - a[3] * (a[1] * a[8] - a[7] * a[2]) + a[6] * (a[1] * a[5] - a[4] * a[2]);
    svd3(a, v, s);
    bool all10 = true, all01 = true;
    for (int k = 0; k < 3; ++k) { const double d = fabs(s[k] - 1.0); all10 = all10 && d >= 0.1; all01 = all01 && d >= 0.01; }
    *det_out = det;
    return det <= 0.0 ? 3 : (all10 ? 2 : (all01 ? 1 : 0));
}
// IRLS_GM.m:92: P = U * round(S) * V' of the SVD irls_edge_status left in a, v, s
__device__ __forceinline__ void irls_edge_project(const double a[9], const double v[9], const double s[3], double* P9) {
    double out[9];
    for (int k = 0; k < 9; ++k) out[k] = 0.0;
    for (int k = 0; k < 3; ++k) {                                                  // U * round(S) * V'
        if (!(s[k] > 0.0)) continue;
        const double rs = round(s[k]);
        for (int r = 0; r < 3; ++r) {
            const double ur = (a[3 * k + r] / s[k]) * rs;
            for (int c = 0; c < 3; ++c) out[r + 3 * c] += ur * v[3 * k + c];
        }
    }
    for (int k = 0; k < 9; ++k) P9[k] = out[k];
}

// ---- stage 4: l1decode_pd, three coordinates batched ---------------------------------------------------------------------------------
struct Pd3 { double tau[3], s[3], ymax[3]; int act[3]; };      // per-coordinate scalars of one launch (act: 1 = this coordinate takes part)

// :268-276 with x0 = 0 at element k = 3 e + c: Ax = 0, u, fu1, fu2, lamu1, lamu2; ev = lamu1 - lamu2 (for Atv, :278)
__device__ __forceinline__ void pd_init_at(const double* y, double ymax, int64_t k, double* Ax, double* u, double* f1, double* f2, double* l1,
                                           double* l2, double* ev) {
    const double ax = 0.0, yy = y[k];
    const double uu = 0.95 * fabs(yy - ax) + 0.10 * ymax;
    const double g1 = (ax - yy) - uu, g2 = (-ax + yy) - uu;
    const double m1 = -1.0 / g1, m2 = -1.0 / g2;
    Ax[k] = ax; u[k] = uu; f1[k] = g1; f2[k] = g2; l1[k] = m1; l2[k] = m2; ev[k] = m1 - m2;
}
// One CSR row of A' v by the 16 lanes of a DPP row (as rhs_row16): g[c] = sum_t sg * ev1, MODE 1 also h[c] = sum_t sg * ev2; MODE 2
// takes sg = 1 (the Jacobi diagonal of A' diag(ev1) A).  Every lane returns the row's totals; an idle row passes t0 = t1.
template <int MODE>
__device__ __forceinline__ void pd_gather_row16(const int32_t* eid, const int8_t* sgn, const double* ev1, const double* ev2, int t0, int t1, int l16,
                                                double* g, double* h) {
    g[0] = g[1] = g[2] = 0; h[0] = h[1] = h[2] = 0;
    for (int t = t0 + l16; t < t1; t += 16) {
        const int64_t e = eid[t];
        const double sg = MODE == 2 ? 1.0 : (double)sgn[t];
        for (int c = 0; c < 3; ++c) {
            g[c] += sg * ev1[3 * e + c];
            if (MODE == 1) h[c] += sg * ev2[3 * e + c];
        }
    }
    for (int c = 0; c < 3; ++c) { g[c] = group16_sum(g[c]); if (MODE == 1) h[c] = group16_sum(h[c]); }
}
// what the row writes: MODE 1 coef .* (A' ev1) - A' ev2 (w1p, :303-304), else the sum itself
template <int MODE>
__device__ __forceinline__ double pd_gather_out(double coef, double g, double h) { return MODE == 1 ? coef * g - h : g; }
// :296-304 at element k of coordinate c: w2, sig1, sig2, sigx; ev1 = -1./fu1 + 1./fu2 (w1), ev2 = (sig2./sig1).*w2 (w1p).  A coordinate
// not taking part gets sigx = 1 and zero right-hand sides: its CG ends at once.
__device__ __forceinline__ void pd_pre_at(const Pd3& a, int c, int64_t k, const double* f1, const double* f2, const double* l1, const double* l2,
                                          double* w2, double* s1, double* s2, double* sx, double* ev1, double* ev2) {
    if (!a.act[c]) { sx[k] = 1.0; ev1[k] = 0.0; ev2[k] = 0.0; return; }
    const double g1 = f1[k], g2 = f2[k], m1 = l1[k], m2 = l2[k], it = 1.0 / a.tau[c];
    const double ww = -1.0 - it * (1.0 / g1 + 1.0 / g2);                     // :296
    const double a1 = -m1 / g1 - m2 / g2;                                    // :298
    const double a2 = m1 / g1 - m2 / g2;                                     // :299
    const double ax = a1 - a2 * a2 / a1;                                     // :300
    w2[k] = ww; s1[k] = a1; s2[k] = a2; sx[k] = ax;
    ev1[k] = -1.0 / g1 + 1.0 / g2;                                           // :303
    ev2[k] = (a2 / a1) * ww;                                                 // :304
}
// :315-324 at coordinate c of edge e = (i, j): Adx, du, dlamu1, dlamu2; ev = dlamu1 - dlamu2 (Atdv); the two step-length minima
// (:327-330; MATLAB's min skips NaN, so does fmin) into mn[c] (lamu bound) and mn[3 + c] (fu bound)
__device__ __forceinline__ void pd_dir_at(const Pd3& a, int c, int64_t e, int i, int j, const double* dx, const double* f1, const double* f2,
                                          const double* l1, const double* l2, const double* w2, const double* s1, const double* s2, double* Adx,
                                          double* du, double* d1, double* d2, double* ev, double* mn) {
    const int64_t k = 3 * e + c;
    if (!a.act[c]) { ev[k] = 0.0; return; }
    const double adx = (j > 0 ? dx[3 * j + c] : 0.0) - (i > 0 ? dx[3 * i + c] : 0.0);
    const double it = 1.0 / a.tau[c], g1 = f1[k], g2 = f2[k], m1 = l1[k], m2 = l2[k];
    const double dd = (w2[k] - s2[k] * adx) / s1[k];                                 // :318
    const double q1 = -(m1 / g1) * (adx - dd) - m1 - it * 1.0 / g1;                   // :320
    const double q2 = (m2 / g2) * (adx + dd) - m2 - it * 1.0 / g2;                    // :321
    Adx[k] = adx; du[k] = dd; d1[k] = q1; d2[k] = q2; ev[k] = q1 - q2;
    if (q1 < 0) mn[c] = fmin(mn[c], -m1 / q1);                                        // :325-326
    if (q2 < 0) mn[c] = fmin(mn[c], -m2 / q2);
    if ((adx - dd) > 0) mn[3 + c] = fmin(mn[3 + c], -g1 / (adx - dd));               // :327-328
    if ((-adx - dd) > 0) mn[3 + c] = fmin(mn[3 + c], -g2 / (-adx - dd));
}
// the term of element k (coordinate c, taking part) in |[rdual; rcent]|^2 (:280-283, :334-336, :347-349).  TRIAL: of the trial point at
// step a.s (state + s * direction); else of the state itself.  rdual = gradf0 + [Atv; -lamu1 - lamu2], rcent = [-lamu1.*fu1;
// -lamu2.*fu2] - 1/tau.
template <bool TRIAL>
__device__ __forceinline__ double pd_resid_edge(const Pd3& a, int c, int64_t k, const double* y, const double* Ax, const double* u, const double* l1,
                                                const double* l2, const double* Adx, const double* du, const double* d1, const double* d2) {
    double ax = Ax[k], uu = u[k], m1 = l1[k], m2 = l2[k];
    if (TRIAL) { const double s = a.s[c]; uu = u[k] + s * du[k]; ax = Ax[k] + s * Adx[k]; m1 = l1[k] + s * d1[k]; m2 = l2[k] + s * d2[k]; }
    const double g1 = (ax - y[k]) - uu, g2 = (-ax + y[k]) - uu;
    const double it = 1.0 / a.tau[c];
    const double rd = 1.0 + (-m1 - m2);
    const double r1 = -m1 * g1 - it, r2 = -m2 * g2 - it;
    return rd * rd + r1 * r1 + r2 * r2;
}
// the term of node v >= 1 in the same sum: Atv (TRIAL: + s * Atdv) squared
template <bool TRIAL>
__device__ __forceinline__ double pd_resid_node(const Pd3& a, int c, int v, const double* Atv, const double* Atdv) {
    const double t = TRIAL ? Atv[3 * v + c] + a.s[c] * Atdv[3 * v + c] : Atv[3 * v + c];
    return t * t;
}
// the accepted step (:340-344) at element k of a coordinate with act set
__device__ __forceinline__ void pd_accept_at(const Pd3& a, int c, int64_t k, const double* y, double* Ax, double* u, double* l1, double* l2, double* f1,
                                             double* f2, const double* Adx, const double* du, const double* d1, const double* d2) {
    const double s = a.s[c];
    const double uu = u[k] + s * du[k], ax = Ax[k] + s * Adx[k], m1 = l1[k] + s * d1[k], m2 = l2[k] + s * d2[k];
    const double g1 = (ax - y[k]) - uu, g2 = (-ax + y[k]) - uu;
    u[k] = uu; Ax[k] = ax; l1[k] = m1; l2[k] = m2; f1[k] = g1; f2[k] = g2;
}
// and at node v: x and Atv move along dx and Atdv
__device__ __forceinline__ void pd_accept_node(const Pd3& a, int c, int v, double* x, double* Atv, const double* dx, const double* Atdv) {
    x[3 * v + c] = x[3 * v + c] + a.s[c] * dx[3 * v + c]; Atv[3 * v + c] = Atv[3 * v + c] + a.s[c] * Atdv[3 * v + c];
}

// BoxMedianSO3Graph.m:172-185 for one node: the exp map of the solved tangent vector (NaN -> 0), Q <- Q * W; returns |W_v|, the node's
// term of the score (a maximum over v >= 1)
__device__ __forceinline__ double l1_node_update(const double* x3, Quat* q) {
    double theta;
    const Quat w = qexp(x3[0], x3[1], x3[2], &theta);
    *q = qmul(*q, w);
    return theta;
}
// RobustMeanSO3Graph.m:169-170 (GM) / L12.m:169-171 from the squared residual s of an edge; mode: DESC_IRLS_GM or DESC_IRLS_L12
__device__ __forceinline__ double irls_weight(double s, int mode, double sigma) {
    double wt;
    if (mode == DESC_IRLS_GM) wt = sigma / (s + sigma * sigma);
    else { wt = 1.0 / pow(sqrt(s), 0.75); if (wt > 1e4) wt = 1e4; }
    return wt;
}

// ---- the scalar rules of l1decode_pd (:262-266, :280-287, :325-350) and of the two outer loops: taken on the host by irls.hip, inside
// the workgroup by irls_batch.hip
constexpr int PD_RG = 256;             // blocks of the partial-reduction kernels: partials are [PD_RG][K], summed in block order from 0.0
// The Newton-system CG is probed every PD_PROBE steps: the reported step count is the solve's true count rounded up to a multiple of it.
constexpr int PD_PROBE = 5;
constexpr int PD_MAX_BACKITER = 32;    // :339
constexpr double PD_TOL = 2.220446049250313e-16, PD_ALPHA = 0.01, PD_BETA = 0.5, PD_MU = 10.0;   // :262-266

// sdg = -(fu1'*lamu1 + fu2'*lamu2), tau = mu * 2 M / sdg (:280-281, :347-348)
__host__ __device__ __forceinline__ double pd_sdg(double dot1, double dot2) { return -(dot1 + dot2); }
__host__ __device__ __forceinline__ double pd_tau(double M, double sdg) { return PD_MU * 2.0 * M / sdg; }
__host__ __device__ __forceinline__ double pd_resnorm(double rr) { return sqrt(rr); }
// :287, :350: the coordinate goes on
__host__ __device__ __forceinline__ int pd_goes_on(double sdg, int pditer, int pdmaxiter) { return !((sdg < PD_TOL) | (pditer >= pdmaxiter)); }
// w1 = -1/tau * (A' ...): the coefficient of k_pd_gather<1>
__host__ __device__ __forceinline__ double pd_gather_coef(int run, double tau) { return run ? -1.0 / tau : 0.0; }
// :325-330: s = 0.99 * min(1, the lamu bound, the fu bound)
__host__ __device__ __forceinline__ double pd_step_length(double mn_lam, double mn_fu) {
    double s = fmin(1.0, mn_lam);
    s = 0.99 * fmin(s, mn_fu);
    return s;
}
// One backtracking trial of a searching coordinate (:332-346) from the trial point's |r|^2: PD_TRIAL_ACCEPT the step *s is taken,
// PD_TRIAL_STUCK the 32-trial limit is passed, PD_TRIAL_AGAIN another trial; *s is halved and *backiter counted in every case.
enum { PD_TRIAL_AGAIN = 0, PD_TRIAL_ACCEPT = 1, PD_TRIAL_STUCK = 2 };
__host__ __device__ __forceinline__ int pd_trial(double rr, double resnorm, double* s, int* backiter, double* s_tried) {
    const bool suffdec = sqrt(rr) <= (1.0 - PD_ALPHA * *s) * resnorm;
    *s_tried = *s;
    *s = PD_BETA * *s;
    ++*backiter;
    if (*backiter > PD_MAX_BACKITER) return PD_TRIAL_STUCK;                             // :339-343
    return suffdec ? PD_TRIAL_ACCEPT : PD_TRIAL_AGAIN;
}
// BoxMedianSO3Graph.m:138-139: the L1 loop's condition, and its L1Step / changeThreshold rule at the head of an iteration
__host__ __device__ __forceinline__ bool l1_goes_on(double score, double changeThreshold, int L1Step, int Iteration, int max_l1) {
    return ((score >= changeThreshold) || (L1Step < 2)) && (Iteration < max_l1);
}
__host__ __device__ __forceinline__ void l1_step_rule(double score, double* changeThreshold, int* L1Step) {
    if (score < *changeThreshold) { *L1Step = *L1Step * 4; *changeThreshold = *changeThreshold / 100; }
}
// RobustMeanSO3Graph.m:130
__host__ __device__ __forceinline__ bool irls_goes_on(double score, int Iteration, int max_irls) { return (score > 1e-3) && (Iteration < max_irls); }
// BoxMedianSO3Graph.m:93-95, :101-103: one entry 2 e + dir of the tree sequence with g = QQ_e: dir 0 Q(j) = QQ * Q(i), dir 1 Q(i) from Q(j)
__host__ __device__ __forceinline__ void irls_tree_step(int32_t entry, const Quat& g, const int32_t* ii, const int32_t* jj, Quat* Q) {
    const int e = entry >> 1;
    if ((entry & 1) == 0) Q[jj[e]] = qmul(g, Q[ii[e]]);
    else Q[ii[e]] = qmul(Quat{-g.a, g.x, g.y, g.z}, Q[jj[e]]);
}

// BoxMedianSO3Graph.m:79-114, the graph part: passes over the edges in `visit` order (the caller's rows) from node 0 until every node
// is reached; seq gets one entry 2 e + dir per reached node, in the order the reference sets them: dir 0 Q(j) = QQ_e * Q(i), dir 1
// Q(i) from Q(j).  Returns the number of nodes reached (n when the graph is connected).
template <class Vec>
inline int64_t irls_tree_sequence(int64_t n, const int32_t* ii, const int32_t* jj, const int32_t* visit, int64_t m, Vec& seq) {
    std::vector<uint8_t> done((size_t)n, 0);
    seq.clear();
    done[0] = 1;                                                                            // :86-87 (a = 1)
    int64_t count = 1;
    while (count < n) {
        bool span = false;
        for (int64_t t = 0; t < m; ++t) {
            const int32_t e = visit[t];
            const int i = ii[e], j = jj[e];
            if (done[i] && !done[j]) { seq.push_back(2 * e); done[j] = 1; ++count; span = true; }
            if (!done[i] && done[j]) { seq.push_back(2 * e + 1); done[i] = 1; ++count; span = true; }
        }
        if (!span) break;
    }
    return count;
}

}  // namespace desc

// IRLS_GM / IRLS_L12 (Algorithms/IRLS_GM.m, IRLS_L12.m; Chatterjee & Govindu, "Efficient and robust large-scale rotation averaging").
//   :52-53    RR = permute(RijMat, [2,1,3]), I = Ind'
//   :65-67    largest connected component (components_device, mst.hip); sub-problem uploaded only when the graph is not connected
//   :82-93    per-edge checks and projection RR = U round(S) V' (k_irls_project: 3x3 one-sided Jacobi SVD)
//   :94-96    BoxMedianSO3Graph (Utils/BoxMedianSO3Graph.m): spanning-tree start (:79-114, host pass in the caller's row order),
//             L1 loop (:138-187) with three l1decode_pd solves per iteration (:245-360), batched here: all state in HBM as m x 3
//             edge and n x 3 node arrays, the averaging core's Jacobi-PCG (laa_pcg) for the three Newton systems A' diag(sigx_c) A dx_c = w1p_c
//   :96       RobustMeanSO3Graph (GM) or L12 (L 1/2): Weighted_LAA steps (laa.h, laa.hip), then residual-and-weight kernel
// Deviations from the reference, by necessity:
//   * graphconncomp's component numbering cannot be checked here: a tie of maximal sizes goes to the component holding the smallest
//     node id (assumed to be graphconncomp's first); with distinct sizes nothing depends on it.
//   * linsolve's LU and its rcond (hcond < 1e-14 -> "Matrix ill-conditioned") are a CG: the ill-conditioned return is taken on a CG
//     breakdown (a non-finite p'Hp or r'z, or p'Hp <= 0 while r'z > 0).  A solve stopping at the iteration cap is counted in
//     cg_unconverged and warned about.  A coordinate whose right-hand side is all zero makes the reference divide by zero (u = 0)
//     and return its start 0 after "Stuck backtracking"; here the NaNs end it one way or the other, also with 0.
//   * The primal-dual step scalars (tau, sdg, resnorm, step length) are formed on the host from fixed-order device partials, one
//     read-back per backtracking trial; the CG keeps its scalars on the device and is probed every PD_PROBE = 5 steps.
// Reductions are fixed-order partials (no float atomics): results are bitwise reproducible from run to run.
// The per-element arithmetic of the kernels below and the scalar rules of pd_solve and the two outer loops are the text of irls_math.h,
// which the batched call (irls_batch.hip) runs too: a change there changes both paths together.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "irls_math.h"
#include "laa.h"

namespace desc {
namespace {

constexpr int RG = PD_RG;         // blocks of the partial-reduction kernels: partials are [RG][K], summed on the host in block order

// ---- stage 3: per-edge checks and projection (the per-edge text: irls_math.h) -------------------------------------------------------
// IRLS_GM.m:82-93 for every edge: P = U round(S) V' of RR = Rij' (column-major, RR orientation).  status: 3 det <= 0, 2 all three
// |s - 1| >= 0.1, 1 all three >= 0.01 (warning), 0 fine.  The smallest failing caller row goes to *bad_row (integer atomicMin),
// warnings are counted.  only >= 0: that edge alone, its status / det / s into info[5].
__global__ __launch_bounds__(256) void k_irls_project(const double* rij, const int32_t* order, int64_t m, double* P, int32_t* bad_row,
                                                      int32_t* warn, int64_t only, double* info) {
    const int64_t lo = only >= 0 ? only : 0, hi = only >= 0 ? only + 1 : m;
    for (int64_t e = lo + (int64_t)blockIdx.x * 256 + threadIdx.x; e < hi; e += (int64_t)gridDim.x * 256) {
        double a[9], v[9], s[3], det;
        const int status = irls_edge_status(rij + 9 * e, a, v, s, &det);
        if (only >= 0) {
            info[0] = status; info[1] = det; info[2] = s[0]; info[3] = s[1]; info[4] = s[2];
            continue;
        }
        const int32_t row = order ? order[e] : (int32_t)e;
        if (status >= 2) atomicMin(bad_row, row);
        else if (status == 1) atomicAdd(warn, 1);
        irls_edge_project(a, v, s, P + 9 * e);
    }
}

// ---- stage 4: l1decode_pd, three coordinates batched (the per-element text: irls_math.h) ---------------------------------------------
// max |y - Ax| with Ax = 0 (:271): MATLAB's max, per coordinate
__global__ __launch_bounds__(256) void k_pd_absmax(const double* y, int64_t m, double* part) {
    double v[3] = {0, 0, 0};
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256)
        for (int c = 0; c < 3; ++c) v[c] = fmax(v[c], fabs(y[3 * e + c]));
    block_reduce<3, 2>(v, part + 3 * blockIdx.x);
}
// :268-276 with x0 = 0: Ax = 0, u, fu1, fu2, lamu1, lamu2; ev = lamu1 - lamu2 (for Atv, :278)
__global__ __launch_bounds__(256) void k_pd_init(const double* y, int64_t m, Pd3 a, double* Ax, double* u, double* f1, double* f2, double* l1,
                                                 double* l2, double* ev) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256)
        for (int c = 0; c < 3; ++c) pd_init_at(y, a.ymax[c], 3 * e + c, Ax, u, f1, f2, l1, l2, ev);
}
// A' v over the CSR rows (16 lanes per row, as k_rhs): MODE 0 out = A' ev1; MODE 1 out = coef .* (A' ev1) - A' ev2 (w1p, :303-304);
// MODE 2 out = sum of ev1 over the row (the Jacobi diagonal of A' diag(ev1) A).  Row 0 (node 1, grounded) is 0.
template <int MODE>
__global__ __launch_bounds__(256) void k_pd_gather(const int32_t* rowptr, const int32_t* eid, const int8_t* sgn, const double* ev1,
                                                   const double* ev2, Pd3 a, double* out, int n) {
    const int l16 = threadIdx.x & 15;
    const int row0 = (blockIdx.x * 256 + threadIdx.x) >> 4, nrows = (gridDim.x * 256) >> 4;
    for (int vb = row0 - (row0 % 4); vb < n; vb += nrows) {
        const int v = vb + (row0 % 4);
        const bool on = v < n && v > 0;
        double g[3], h[3];
        pd_gather_row16<MODE>(eid, sgn, ev1, ev2, on ? rowptr[v] : 0, on ? rowptr[v + 1] : 0, l16, g, h);
        if (v < n && l16 == 0)
            for (int c = 0; c < 3; ++c) out[3 * v + c] = pd_gather_out<MODE>(a.tau[c], g[c], h[c]);
    }
}
// :296-304 per edge: w2, sig1, sig2, sigx; ev1 = -1./fu1 + 1./fu2 (w1), ev2 = (sig2./sig1).*w2 (w1p).  Coordinates not taking part get
// sigx = 1 and zero right-hand sides: their CG ends at once.
__global__ __launch_bounds__(256) void k_pd_pre(int64_t m, Pd3 a, const double* f1, const double* f2, const double* l1, const double* l2,
                                                double* w2, double* s1, double* s2, double* sx, double* ev1, double* ev2) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256)
        for (int c = 0; c < 3; ++c) pd_pre_at(a, c, 3 * e + c, f1, f2, l1, l2, w2, s1, s2, sx, ev1, ev2);
}
// :315-324: Adx, du, dlamu1, dlamu2; ev = dlamu1 - dlamu2 (Atdv); the two step-length minima (:327-330) as block partials [RG][6]: lamu
// bound per coordinate, then fu bound per coordinate
__global__ __launch_bounds__(256) void k_pd_dir(const int32_t* ii, const int32_t* jj, int64_t m, Pd3 a, const double* dx, const double* f1,
                                                const double* f2, const double* l1, const double* l2, const double* w2, const double* s1,
                                                const double* s2, double* Adx, double* du, double* d1, double* d2, double* ev, double* part) {
    double mn[6] = {INFINITY, INFINITY, INFINITY, INFINITY, INFINITY, INFINITY};
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256) {
        const int i = ii[e], j = jj[e];
        for (int c = 0; c < 3; ++c) pd_dir_at(a, c, e, i, j, dx, f1, f2, l1, l2, w2, s1, s2, Adx, du, d1, d2, ev, mn);
    }
    block_reduce<6, 1>(mn, part + 6 * blockIdx.x);
}
// |[rdual; rcent]|^2 per coordinate as block partials [RG][3] (:280-283, :334-336, :347-349).  TRIAL: of the trial point at step a.s
// (state + s * direction); else of the state itself.
template <bool TRIAL>
__global__ __launch_bounds__(256) void k_pd_resid(int64_t m, int n, Pd3 a, const double* y, const double* Ax, const double* u, const double* l1,
                                                  const double* l2, const double* Atv, const double* Adx, const double* du, const double* d1,
                                                  const double* d2, const double* Atdv, double* part) {
    double acc[3] = {0, 0, 0};
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256)
        for (int c = 0; c < 3; ++c) {
            if (!a.act[c]) continue;
            acc[c] += pd_resid_edge<TRIAL>(a, c, 3 * e + c, y, Ax, u, l1, l2, Adx, du, d1, d2);
        }
    for (int v = blockIdx.x * 256 + threadIdx.x; v < n; v += gridDim.x * 256) {
        if (v == 0) continue;
        for (int c = 0; c < 3; ++c) {
            if (!a.act[c]) continue;
            acc[c] += pd_resid_node<TRIAL>(a, c, v, Atv, Atdv);
        }
    }
    block_reduce<3, 0>(acc, part + 3 * blockIdx.x);
}
// the accepted step (:340-344) for the coordinates with act set (row 0 of x and Atv, the grounded node, is not written), then fu1'*lamu1
// and fu2'*lamu2 of the new point as partials [RG][6]
__global__ __launch_bounds__(256) void k_pd_accept(int64_t m, int n, Pd3 a, const double* y, double* Ax, double* u, double* l1, double* l2,
                                                   double* f1, double* f2, double* x, double* Atv, const double* dx, const double* Adx,
                                                   const double* du, const double* d1, const double* d2, const double* Atdv, double* part) {
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256)
        for (int c = 0; c < 3; ++c) {
            const int64_t k = 3 * e + c;
            if (a.act[c]) pd_accept_at(a, c, k, y, Ax, u, l1, l2, f1, f2, Adx, du, d1, d2);
            acc[c] += f1[k] * l1[k]; acc[3 + c] += f2[k] * l2[k];
        }
    for (int v = blockIdx.x * 256 + threadIdx.x; v < n; v += gridDim.x * 256) {
        if (v == 0) continue;                                                 // the grounded node: x and Atv stay 0
        for (int c = 0; c < 3; ++c)
            if (a.act[c]) pd_accept_node(a, c, v, x, Atv, dx, Atdv);
    }
    block_reduce<6, 0>(acc, part + 6 * blockIdx.x);
}

// BoxMedianSO3Graph.m:172-185: score partial max_v |W_v| (v >= 1), exp map (NaN -> 0), Q <- Q * W.  x row 0 is 0.
__global__ __launch_bounds__(256) void k_l1_node_update(const double* x, Quat* Q, int n, double* part) {
    double sc[1] = {0.0};
    for (int v = blockIdx.x * 256 + threadIdx.x; v < n; v += gridDim.x * 256) {
        const double theta = l1_node_update(x + 3 * v, Q + v);
        if (v > 0) sc[0] = fmax(sc[0], theta);
    }
    block_reduce<1, 2>(sc, part + blockIdx.x);
}

// ---- stage 5: residuals and weights (RobustMeanSO3Graph.m:169-170, L12.m:169-171) from the solved W (before the exp map) --------------
__global__ __launch_bounds__(256) void k_irls_weights(const double* x, const double* B, const int32_t* ii, const int32_t* jj, int64_t m, int mode,
                                                      double sigma, double* w) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256)
        w[e] = irls_weight(edge_residual_sq(x, B, ii, jj, e), mode, sigma);
}
__global__ void k_fill(double* p, int64_t count, double v) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (int64_t)gridDim.x * blockDim.x) p[t] = v;
}
__global__ void k_gather_quat(const Quat* QQ, const int32_t* ids, int count, Quat* out) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < count; t += gridDim.x * blockDim.x) out[t] = QQ[ids[t]];
}

// ---- the L1 stage's batched primal-dual solver ---------------------------------------------------------------------------------------
struct PdState {
    LaaSolver* L = nullptr;
    int64_t n = 0, m = 0;
    int egrid = 1, ngrid = 1, rgrid = 1;
    double *y, *Ax, *u, *f1, *f2, *l1, *l2, *w2, *s1, *s2, *sx, *ev1, *ev2, *Adx, *du, *d1, *d2;     // m x 3
    double *x, *Atv, *w1p, *dg, *dx, *Atdv;                                                          // n x 3 (the PCG works in L's arrays)
    double* part;
    hvec<double> hpart;
    // counters
    int steps = 0, ill = 0, stuck = 0, solves = 0;
    CgCount cg;
    double ms_pcg = 0.0;
    bool verbose = false;
};

// the state arrays in their fixed order (pd_alloc; the snapshot of desc_test_irls_pd_stage): PD_EDGE_ARRAYS of m x 3, PD_NODE_ARRAYS of n x 3
constexpr int PD_EDGE_ARRAYS = 17, PD_NODE_ARRAYS = 6;
struct PdArrays { double** em[PD_EDGE_ARRAYS]; double** nm[PD_NODE_ARRAYS]; };
PdArrays pd_arrays(PdState& S) {
    return {{&S.y, &S.Ax, &S.u, &S.f1, &S.f2, &S.l1, &S.l2, &S.w2, &S.s1, &S.s2, &S.sx, &S.ev1, &S.ev2, &S.Adx, &S.du, &S.d1, &S.d2},
            {&S.x, &S.Atv, &S.w1p, &S.dg, &S.dx, &S.Atdv}};
}

int pd_alloc(PdState& S, LaaSolver& L) {
    int rc = DESC_OK;
    S.L = &L; S.n = L.n; S.m = L.m;
    const int64_t m3 = 3 * S.m, n3 = 3 * S.n;
    const PdArrays arr = pd_arrays(S);
    for (auto* a : arr.em) if ((rc = L.alloc(a, m3))) return rc;
    for (auto* a : arr.nm) if ((rc = L.alloc(a, n3))) return rc;
    if ((rc = L.alloc(&S.part, 6 * RG))) return rc;
    S.hpart.resize(6 * RG);
    S.egrid = L.egrid; S.ngrid = L.ngrid; S.rgrid = L.rgrid;
    return DESC_OK;
}

// fixed-order host sums / minima of [RG][K] partials
int read_part(PdState& S, int K, double* out, bool take_min) {
    DESC_HIP(hipMemcpy(S.hpart.data(), S.part, sizeof(double) * K * RG, hipMemcpyDeviceToHost));
    for (int k = 0; k < K; ++k) {
        double a = take_min ? INFINITY : 0.0;
        for (int b = 0; b < RG; ++b) a = take_min ? std::fmin(a, S.hpart[(size_t)K * b + k]) : a + S.hpart[(size_t)K * b + k];
        out[k] = a;
    }
    return DESC_OK;
}

// dx_c = (A' diag(sx_c) A) \ w1p_c for the coordinates in act; bad[c] set on a breakdown
int pd_pcg(PdState& S, const int act[3], int bad[3]) {
    LaaSolver& L = *S.L;
    Pd3 none{}; none.act[0] = none.act[1] = none.act[2] = 1;
    hipLaunchKernelGGL(k_pd_gather<2>, dim3(S.rgrid), dim3(256), 0, 0, L.dp->d_rowptr, L.dp->d_adj_eid, L.d_sgn, S.sx, nullptr, none, S.dg, (int)S.n);
    ++S.solves;
    return laa_pcg<true, true>(L, S.sx, S.w1p, S.dg, S.dx, act, PD_PROBE, S.cg, bad);
}

// What pd_solve decided, for desc_test_irls_pd_solve: record 0 is the start, record k step k; a record holds PD_TRACE_FIELDS doubles per
// coordinate: takes part, the CG's bad, the first trial step s, the number of trials, the verdict (0 none, PD_TRIAL_ACCEPT, PD_TRIAL_STUCK),
// then sdg, tau, resnorm as they stand after the step.  Filled from values the loop has on the host anyway.
constexpr int PD_TRACE_FIELDS = 8;
struct PdTrace { double* rec = nullptr; int cap = 0, len = 0; };

// W(2:end, 2:4) = [l1decode_pd(0, A, [], B(:,c), eps, pdmaxiter, AtA) for c = 1..3] (BoxMedianSO3Graph.m:166-168) into S.x
int pd_solve(PdState& S, const double* d_B, int pdmaxiter, PdTrace* tr = nullptr) {
    int rc = DESC_OK;
    const LaaSolver& L = *S.L;
    const desc_device_problem* dp = L.dp;
    const int64_t m = S.m;
    const int n = (int)S.n;
    const double M = (double)m;
    DESC_HIP(hipMemcpyAsync(S.y, d_B, sizeof(double) * 3 * m, hipMemcpyDeviceToDevice, 0));
    DESC_HIP(hipMemsetAsync(S.x, 0, sizeof(double) * 3 * n, 0));
    Pd3 a{}; for (int c = 0; c < 3; ++c) a.act[c] = 1;
    // ---- start (:268-287)
    hipLaunchKernelGGL(k_pd_absmax, dim3(RG), dim3(256), 0, 0, S.y, m, S.part);
    {
        DESC_HIP(hipMemcpy(S.hpart.data(), S.part, sizeof(double) * 3 * RG, hipMemcpyDeviceToHost));
        for (int c = 0; c < 3; ++c) { double v = 0.0; for (int b = 0; b < RG; ++b) v = std::fmax(v, S.hpart[3 * b + c]); a.ymax[c] = v; }
    }
    hipLaunchKernelGGL(k_pd_init, dim3(S.egrid), dim3(256), 0, 0, S.y, m, a, S.Ax, S.u, S.f1, S.f2, S.l1, S.l2, S.ev1);
    hipLaunchKernelGGL(k_pd_gather<0>, dim3(S.rgrid), dim3(256), 0, 0, dp->d_rowptr, dp->d_adj_eid, L.d_sgn, S.ev1, nullptr, a, S.Atv, n);
    double tau[3], resnorm[3], sdg[3], dots[6];
    // sdg, tau, resnorm of the current point (:280-283, :347-350) for the coordinates in act; fu1'*lamu1 and fu2'*lamu2 are the
    // partials the last k_pd_accept launch left in S.part (it forms them from the point it has just written)
    auto scalars = [&](const int act[3]) -> int {
        Pd3 b{};
        int rc2 = read_part(S, 6, dots, false);
        if (rc2) return rc2;
        for (int c = 0; c < 3; ++c) {
            if (!act[c]) continue;
            sdg[c] = pd_sdg(dots[c], dots[3 + c]);
            tau[c] = pd_tau(M, sdg[c]);
            b.act[c] = 1; b.tau[c] = tau[c];
        }
        hipLaunchKernelGGL(k_pd_resid<false>, dim3(RG), dim3(256), 0, 0, m, n, b, S.y, S.Ax, S.u, S.l1, S.l2, S.Atv, S.Adx, S.du, S.d1, S.d2,
                           S.Atdv, S.part);
        double rr[3];
        if ((rc2 = read_part(S, 3, rr, false))) return rc2;
        for (int c = 0; c < 3; ++c) if (act[c]) resnorm[c] = pd_resnorm(rr[c]);
        return DESC_OK;
    };
    int run[3] = {1, 1, 1};
    {
        const Pd3 none{};                                                // no coordinate moves: only the dot partials of the start
        hipLaunchKernelGGL(k_pd_accept, dim3(RG), dim3(256), 0, 0, m, n, none, S.y, S.Ax, S.u, S.l1, S.l2, S.f1, S.f2, S.x, S.Atv, S.dx, S.Adx,
                           S.du, S.d1, S.d2, S.Atdv, S.part);
    }
    if ((rc = scalars(run))) return rc;
    int pditer = 0;
    // the trace record of step `pditer` (nullptr: none kept), and its closing fields
    auto record = [&]() -> double* {
        if (!tr || pditer >= tr->cap) return nullptr;
        double* r = tr->rec + (size_t)3 * PD_TRACE_FIELDS * pditer;
        std::fill(r, r + 3 * PD_TRACE_FIELDS, 0.0);
        return r;
    };
    auto close_record = [&](double* r) {
        if (!r) return;
        for (int c = 0; c < 3; ++c) { r[PD_TRACE_FIELDS * c + 5] = sdg[c]; r[PD_TRACE_FIELDS * c + 6] = tau[c]; r[PD_TRACE_FIELDS * c + 7] = resnorm[c]; }
        tr->len = pditer + 1;
    };
    {
        double* r = record();
        if (r) for (int c = 0; c < 3; ++c) r[PD_TRACE_FIELDS * c] = 1.0;
        close_record(r);
    }
    for (int c = 0; c < 3; ++c) run[c] = pd_goes_on(sdg[c], pditer, pdmaxiter);                // :287
    while (run[0] || run[1] || run[2]) {
        ++pditer;
        double* const rec = record();
        if (rec) for (int c = 0; c < 3; ++c) rec[PD_TRACE_FIELDS * c] = run[c];
        for (int c = 0; c < 3; ++c) { a.act[c] = run[c]; a.tau[c] = tau[c]; }
        // ---- Newton system (:296-312)
        hipLaunchKernelGGL(k_pd_pre, dim3(S.egrid), dim3(256), 0, 0, m, a, S.f1, S.f2, S.l1, S.l2, S.w2, S.s1, S.s2, S.sx, S.ev1, S.ev2);
        Pd3 g = a;
        for (int c = 0; c < 3; ++c) g.tau[c] = pd_gather_coef(run[c], tau[c]);                // w1 = -1/tau * (A' ...)
        hipLaunchKernelGGL(k_pd_gather<1>, dim3(S.rgrid), dim3(256), 0, 0, dp->d_rowptr, dp->d_adj_eid, L.d_sgn, S.ev1, S.ev2, g, S.w1p, n);
        DESC_HIP(hipDeviceSynchronize());
        auto tp = std::chrono::steady_clock::now();
        int bad[3];
        if ((rc = pd_pcg(S, run, bad))) return rc;
        S.ms_pcg += ms_since(tp);
        for (int c = 0; c < 3; ++c)
            if (bad[c]) {                                                                    // :308-312
                if (S.verbose) printf("Matrix ill-conditioned.  Returning previous iterate.  (See Section 4 of notes for more information.)\n");
                ++S.ill; run[c] = 0; a.act[c] = 0;
                if (rec) rec[PD_TRACE_FIELDS * c + 1] = 1.0;
            }
        if (!(run[0] || run[1] || run[2])) { close_record(rec); break; }
        for (int c = 0; c < 3; ++c) if (run[c]) ++S.steps;
        // ---- direction and step length (:315-330)
        hipLaunchKernelGGL(k_pd_dir, dim3(RG), dim3(256), 0, 0, dp->d_ii, dp->d_jj, m, a, S.dx, S.f1, S.f2, S.l1, S.l2, S.w2, S.s1, S.s2, S.Adx, S.du,
                           S.d1, S.d2, S.ev1, S.part);
        double mins[6];
        if ((rc = read_part(S, 6, mins, true))) return rc;
        hipLaunchKernelGGL(k_pd_gather<0>, dim3(S.rgrid), dim3(256), 0, 0, dp->d_rowptr, dp->d_adj_eid, L.d_sgn, S.ev1, nullptr, a, S.Atdv, n);
        double s[3] = {0, 0, 0};
        for (int c = 0; c < 3; ++c)
            if (run[c]) { s[c] = pd_step_length(mins[c], mins[3 + c]); if (rec) rec[PD_TRACE_FIELDS * c + 2] = s[c]; }
        // ---- backtracking (:332-346): one trial of every searching coordinate per launch
        int search[3], backiter[3] = {0, 0, 0}, accept[3] = {0, 0, 0};
        double s_acc[3] = {0, 0, 0};
        for (int c = 0; c < 3; ++c) search[c] = run[c];
        while (search[0] || search[1] || search[2]) {
            Pd3 t{};
            for (int c = 0; c < 3; ++c) { t.act[c] = search[c]; t.s[c] = s[c]; t.tau[c] = tau[c]; }
            hipLaunchKernelGGL(k_pd_resid<true>, dim3(RG), dim3(256), 0, 0, m, n, t, S.y, S.Ax, S.u, S.l1, S.l2, S.Atv, S.Adx, S.du, S.d1, S.d2,
                               S.Atdv, S.part);
            double rr[3];
            if ((rc = read_part(S, 3, rr, false))) return rc;
            for (int c = 0; c < 3; ++c) {
                if (!search[c]) continue;
                double s_tried;
                const int verdict = pd_trial(rr[c], resnorm[c], &s[c], &backiter[c], &s_tried);
                if (verdict == PD_TRIAL_STUCK) {                                             // :339-343
                    if (S.verbose) printf("Stuck backtracking, returning last iterate.  (See Section 4 of notes for more information.)\n");
                    ++S.stuck; search[c] = 0; run[c] = 0;
                } else if (verdict == PD_TRIAL_ACCEPT) { search[c] = 0; accept[c] = 1; s_acc[c] = s_tried; }
                if (rec) { rec[PD_TRACE_FIELDS * c + 3] = backiter[c]; rec[PD_TRACE_FIELDS * c + 4] = verdict; }
            }
        }
        // ---- next iterate (:348-356)
        Pd3 acc{};
        for (int c = 0; c < 3; ++c) { acc.act[c] = accept[c]; acc.s[c] = s_acc[c]; }
        hipLaunchKernelGGL(k_pd_accept, dim3(RG), dim3(256), 0, 0, m, n, acc, S.y, S.Ax, S.u, S.l1, S.l2, S.f1, S.f2, S.x, S.Atv, S.dx, S.Adx, S.du,
                           S.d1, S.d2, S.Atdv, S.part);
        if ((rc = scalars(accept))) return rc;
        for (int c = 0; c < 3; ++c)
            if (accept[c]) run[c] = pd_goes_on(sdg[c], pditer, pdmaxiter);
        close_record(rec);
    }
    DESC_HIP(hipGetLastError());
    return DESC_OK;
}

// BoxMedianSO3Graph.m:79-114: the spanning-tree start, passes over the edges in `visit` order; Q n x 4 host quaternions
int tree_start(const desc_device_problem* sp, const hvec<int32_t>& visit, const Quat* d_QQ, hvec<Quat>& Q) {
    const int64_t n = sp->n;
    const int32_t *ii = sp->ii.data(), *jj = sp->jj.data();
    hvec<int32_t> seq, seq_e;
    seq.reserve((size_t)n);
    const int64_t count = irls_tree_sequence(n, ii, jj, visit.data(), (int64_t)visit.size(), seq);
    if (count < n) return fail(DESC_ERR_STATE, "spanning-tree start: %lld of %lld nodes reached", (long long)count, (long long)n);
    for (const int32_t en : seq) seq_e.push_back(en >> 1);
    const int cnt = (int)seq_e.size();
    hvec<Quat> qq((size_t)std::max(cnt, 1));
    if (cnt) {
        DevArena A;                                                                         // freed before the host pass below
        int32_t* d_ids = nullptr; Quat* d_out = nullptr;
        int rc = DESC_OK;
        if ((rc = A.alloc(&d_ids, cnt)) || (rc = A.alloc(&d_out, cnt))) return rc;
        DESC_HIP(hipMemcpy(d_ids, seq_e.data(), sizeof(int32_t) * cnt, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_gather_quat, dim3((cnt + 255) / 256), dim3(256), 0, 0, d_QQ, d_ids, cnt, d_out);
        DESC_HIP(hipMemcpy(qq.data(), d_out, sizeof(Quat) * cnt, hipMemcpyDeviceToHost));
    }
    Q.assign((size_t)n, Quat{1.0, 0.0, 0.0, 0.0});                                          // :78
    for (int t = 0; t < cnt; ++t)
        irls_tree_step(seq[t], qq[t], ii, jj, Q.data());                                    // :93-95, :101-103
    return DESC_OK;
}

struct ProbOwner { desc_device_problem* p = nullptr; ~ProbOwner() { if (p) desc_problem_free(p); } };

}  // namespace
}  // namespace desc

using namespace desc;

extern "C" int desc_irls_run(const desc_problem* prob, const desc_irls_params* params, int32_t device, double* R_out, double* R_l1,
                             desc_irls_info* info) {
    if (!prob || !params || !R_out) return fail(DESC_ERR_INVALID, "NULL argument");
    auto t0 = std::chrono::steady_clock::now();
    const int rc = with_uploaded(prob, device, [&](const desc_device_problem* dp) { return desc_irls_run_dev(dp, params, R_out, R_l1, info); });
    if (!rc && info) info->ms_total = ms_since(t0);
    return rc;
}

extern "C" int desc_irls_run_dev(const desc_device_problem* dp, const desc_irls_params* P, double* R_out, double* R_l1, desc_irls_info* info) {
    return no_throw("desc_irls_run_dev", [&]() -> int {
    if (!dp || !P || !R_out) return fail(DESC_ERR_INVALID, "NULL argument");
    if (P->mode != DESC_IRLS_GM && P->mode != DESC_IRLS_L12) return fail(DESC_ERR_INVALID, "mode must be DESC_IRLS_GM or DESC_IRLS_L12");
    const int64_t n = dp->n, m = dp->m;
    if (n < 2 || m < 1) return fail(DESC_ERR_INVALID, "empty graph");
    const int max_l1 = P->max_iter_l1 > 0 ? P->max_iter_l1 : 10, max_irls = P->max_iter_irls > 0 ? P->max_iter_irls : 100;
    const double sigma = (P->sigma_deg > 0 ? P->sigma_deg : 5.0) * M_PI / 180.0;            // RobustMeanSO3Graph.m:60
    const bool verbose = P->verbose != 0;
    int rc = DESC_OK;
    if (P->order) {
        hvec<uint8_t> seen((size_t)m, 0);
        for (int64_t e = 0; e < m; ++e) {
            const int32_t r = P->order[e];
            if (r < 0 || r >= m || seen[r]) return fail(DESC_ERR_INVALID, "order must be a permutation of 0..m-1");
            seen[r] = 1;
        }
    }
    DESC_HIP(hipSetDevice(dp->device));
    auto t0 = std::chrono::steady_clock::now();
    desc_irls_info I{};
    // ---- stage 3: checks and projection of every edge (IRLS_GM.m:82-93)
    double* d_P = nullptr;
    int32_t *d_flags = nullptr, *d_order = nullptr;
    double* d_einfo = nullptr;
    DevArena A;
    if ((rc = A.alloc(&d_P, 9 * m)) || (rc = A.alloc(&d_flags, 2)) || (rc = A.alloc(&d_einfo, 5)) || (P->order && (rc = A.alloc(&d_order, m)))) return rc;
    if (P->order) DESC_HIP(hipMemcpy(d_order, P->order, sizeof(int32_t) * m, hipMemcpyHostToDevice));
    const int32_t init_flags[2] = {INT_MAX, 0};
    DESC_HIP(hipMemcpy(d_flags, init_flags, sizeof init_flags, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_irls_project, dim3(grid_for(m, 2048)), dim3(256), 0, 0, dp->d_rij, d_order, m, d_P, d_flags, d_flags + 1, (int64_t)-1, d_einfo);
    DESC_HIP(hipGetLastError());
    int32_t flags[2];
    DESC_HIP(hipMemcpy(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost));
    if (flags[0] != INT_MAX) {
        int64_t e = flags[0];
        if (P->order) for (int64_t t = 0; t < m; ++t) if (P->order[t] == flags[0]) { e = t; break; }
        hipLaunchKernelGGL(k_irls_project, dim3(1), dim3(256), 0, 0, dp->d_rij, d_order, m, d_P, d_flags, d_flags + 1, e, d_einfo);
        double ei[5];
        DESC_HIP(hipMemcpy(ei, d_einfo, sizeof ei, hipMemcpyDeviceToHost));
        if (ei[0] == 3) return fail(DESC_ERR_INVALID, "det(RR(:,:,%d))=%f", (int)flags[0] + 1, ei[1]);
        return fail(DESC_ERR_INVALID, "svd(RR(:,:,%d))=[%f %f %f]", (int)flags[0] + 1, ei[2], ei[3], ei[4]);
    }
    I.warned_edges = flags[1];
    if (flags[1]) fprintf(stderr, "[desc_amd] warning: %d edge rotations have all three singular values off 1 by >= 0.01: projected to SO(3)\n", flags[1]);
    I.ms_project = ms_since(t0);
    // ---- stage 2: the largest connected component (IRLS_GM.m:65-67)
    auto t1 = std::chrono::steady_clock::now();
    hvec<int32_t> comp((size_t)n);
    int64_t ncomp = 0;
    if ((rc = components_device(dp, comp.data(), &ncomp))) return rc;
    const desc_device_problem* sp = dp;
    ProbOwner sub;
    const double* d_blocks = d_P;
    hvec<int32_t> nodes, edge_map;                                                          // sub-problem node -> node, edge -> edge
    hvec<int32_t> visit;                                                                    // sub-problem edges in the caller's row order
    if (ncomp > 1) {
        hvec<int64_t> size((size_t)n, 0);
        for (int64_t v = 0; v < n; ++v) ++size[comp[v]];
        hvec<uint8_t> seen((size_t)n, 0);
        int32_t best = -1; int64_t best_size = 0;
        for (int64_t v = 0; v < n; ++v) {                                                    // components by their smallest node: first of max size
            const int32_t l = comp[v];
            if (seen[l]) continue;
            seen[l] = 1;
            if (size[l] > best_size) { best_size = size[l]; best = l; }
        }
        hvec<int32_t> newid((size_t)n, -1);
        for (int64_t v = 0; v < n; ++v) if (comp[v] == best) { newid[v] = (int32_t)nodes.size(); nodes.push_back((int32_t)v); }
        hvec<int32_t> si, sj;
        for (int64_t e = 0; e < m; ++e)
            if (comp[dp->ii[e]] == best) { edge_map.push_back((int32_t)e); si.push_back(newid[dp->ii[e]]); sj.push_back(newid[dp->jj[e]]); }
        const int64_t ms = (int64_t)edge_map.size();
        hvec<double> hP((size_t)9 * m), sP((size_t)9 * ms);
        DESC_HIP(hipMemcpy(hP.data(), d_P, sizeof(double) * 9 * m, hipMemcpyDeviceToHost));
        for (int64_t t = 0; t < ms; ++t) std::copy(&hP[9 * (size_t)edge_map[t]], &hP[9 * (size_t)edge_map[t]] + 9, &sP[9 * (size_t)t]);
        desc_problem q{(int64_t)nodes.size(), ms, si.data(), sj.data(), sP.data()};
        if ((rc = desc_problem_upload(&q, dp->device, &sub.p))) return rc;
        sp = sub.p; d_blocks = sub.p->d_rij;
        visit.resize((size_t)ms);
        for (int64_t t = 0; t < ms; ++t) visit[t] = (int32_t)t;
        if (P->order) std::sort(visit.begin(), visit.end(), [&](int32_t a, int32_t b) { return P->order[edge_map[a]] < P->order[edge_map[b]]; });
    } else {
        visit.resize((size_t)m);
        if (P->order) for (int64_t e = 0; e < m; ++e) visit[P->order[e]] = (int32_t)e;
        else for (int64_t e = 0; e < m; ++e) visit[e] = (int32_t)e;
    }
    const int64_t nc = sp->n, mc = sp->m;
    I.comp_nodes = nc; I.comp_edges = mc;
    I.ms_components = ms_since(t1);
    // ---- stage 4: BoxMedianSO3Graph (IRLS_GM.m:95)
    auto t2 = std::chrono::steady_clock::now();
    hvec<double> r_l1((size_t)9 * nc);
    {
        hvec<double> rinit((size_t)9 * nc, 0.0);
        if (P->R_init) {
            for (int64_t v = 0; v < nc; ++v) {
                const int64_t src = nodes.empty() ? v : nodes[v];
                std::copy(P->R_init + 9 * src, P->R_init + 9 * src + 9, &rinit[9 * (size_t)v]);
            }
        } else
            for (int64_t v = 0; v < nc; ++v) rinit[9 * v] = rinit[9 * v + 4] = rinit[9 * v + 8] = 1.0;
        LaaSolver L;
        if ((rc = laa_setup(sp, rinit.data(), L))) return rc;                              // Q = R2Q(Rinit) (:64-69) when given
        laa_set_qq(L, d_blocks);                                                            // QQ of the projected RR (:55-59)
        if (!P->R_init) {
            auto tt = std::chrono::steady_clock::now();
            hvec<Quat> Q;
            if ((rc = tree_start(sp, visit, L.d_QQ, Q))) return rc;
            DESC_HIP(hipMemcpy(L.d_Q, Q.data(), sizeof(Quat) * nc, hipMemcpyHostToDevice));
            I.ms_tree = ms_since(tt);
        }
        PdState S;
        S.verbose = verbose;
        if ((rc = pd_alloc(S, L))) return rc;
        double* d_smax = nullptr;
        if ((rc = L.alloc(&d_smax, L.sgrid))) return rc;
        hvec<double> smax((size_t)L.sgrid);
        double changeThreshold = .001, score = INFINITY;                                     // :56, :134
        int Iteration = 0, L1Step = 2;
        if (verbose) printf("Itr\tMaxChange\tTime\n%d  NaN  %g\n", 0, ms_since(t2) / 1e3);  // :136-137
        while (l1_goes_on(score, changeThreshold, L1Step, Iteration, max_l1)) {             // :138
            l1_step_rule(score, &changeThreshold, &L1Step);                                 // :139
            laa_edge_log(L);                                                                // :141-160
            if ((rc = pd_solve(S, L.d_B, L1Step))) return rc;                               // :162-168
            hipLaunchKernelGGL(k_l1_node_update, dim3(L.sgrid), dim3(256), 0, 0, S.x, L.d_Q, (int)nc, d_smax);   // :173-185
            DESC_HIP(hipMemcpy(smax.data(), d_smax, sizeof(double) * L.sgrid, hipMemcpyDeviceToHost));
            score = 0.0;
            for (double v : smax) score = std::fmax(score, v);
            ++Iteration;
            if (verbose) printf("%d  %g  %g\n", Iteration, score, ms_since(t2) / 1e3);      // :188
        }
        if (verbose && Iteration >= max_l1) printf("Max iterations reached\n");              // :201
        if ((rc = laa_finish(L, Iteration, r_l1.data()))) return rc;                         // real(q2R(Q)) (:192-197)
        I.l1_iters = Iteration; I.l1_score = score;
        I.pd_steps = S.steps; I.pd_ill = S.ill; I.pd_stuck = S.stuck; I.pd_solves = S.solves;
        I.cg_iters_l1 = S.cg.total; I.cg_unconverged = S.cg.unconverged; I.cg_residual = S.cg.worst; I.ms_l1_pcg = S.ms_pcg;
        if (S.cg.unconverged)
            fprintf(stderr, "[desc_amd] warning: %d primal-dual Newton solves stopped at the PCG iteration cap (relative residual up to %.3e)\n",
                    S.cg.unconverged, S.cg.worst);
    }
    I.ms_l1 = ms_since(t2);
    // ---- stage 5: RobustMeanSO3Graph / L12 (IRLS_GM.m:96)
    auto t3 = std::chrono::steady_clock::now();
    hvec<double> r_out((size_t)9 * nc);
    {
        LaaSolver L;
        if ((rc = laa_setup(sp, r_l1.data(), L))) return rc;                                // Q = R2Q(R) (:75-80)
        laa_set_qq(L, d_blocks);
        hipLaunchKernelGGL(k_fill, dim3(L.egrid), dim3(256), 0, 0, L.d_w, mc, 1.0);         // :127
        double score = INFINITY;
        int Iteration = 0;
        if (verbose) printf("%d  NaN  %g\n", 0, ms_since(t3) / 1e3);                        // :129
        while (irls_goes_on(score, Iteration, max_irls)) {                                  // :130
            if ((rc = laa_step(L, &score))) return rc;                                      // :132-186
            hipLaunchKernelGGL(k_irls_weights, dim3(L.egrid), dim3(256), 0, 0, L.d_x, L.d_B, sp->d_ii, sp->d_jj, mc, P->mode, sigma, L.d_w);   // :169-171
            DESC_HIP(hipGetLastError());
            ++Iteration;
            if (verbose) printf("%d  %g  %g\n", Iteration, score, ms_since(t3) / 1e3);       // :189
        }
        if (verbose && Iteration >= max_irls) printf("Max iterations reached\n");            // :202
        if ((rc = laa_finish(L, Iteration, r_out.data()))) return rc;                        // q2R (:193-197)
        I.irls_iters = Iteration; I.irls_score = score;
        I.cg_iters_irls = L.cg.total; I.cg_unconverged += L.cg.unconverged; I.cg_residual = std::max(I.cg_residual, L.cg.worst);
    }
    I.ms_irls = ms_since(t3);
    // ---- NaN outside the component (:94)
    auto place = [&](const hvec<double>& src, double* dst) {
        if (nodes.empty()) { std::copy(src.begin(), src.end(), dst); return; }
        std::fill(dst, dst + 9 * n, NAN);
        for (size_t v = 0; v < nodes.size(); ++v) std::copy(&src[9 * v], &src[9 * v] + 9, dst + 9 * (int64_t)nodes[v]);
    };
    place(r_out, R_out);
    if (R_l1) place(r_l1, R_l1);
    if (verbose) fflush(stdout);
    I.ms_total = ms_since(t0);
    if (info) *info = I;
    return DESC_OK;
    });
}

// ---- test hooks (include/desc_amd.h, tests/test_gpu_laa_maps.py): the kernels of this file that belong to the averaging core's
// arithmetic, one at a time on caller (host) arrays, launched as desc_irls_run_dev launches them.  Nothing in the library calls them.
extern "C" int desc_test_irls_project(const double* rij, const int32_t* order, int64_t m, int64_t only, int32_t device, double* P,
                                      int32_t* bad_row, int32_t* warn, double* info) {
    return no_throw("desc_test_irls_project", [&]() -> int {
    if (!rij || !P || !bad_row || !warn || !info) return fail(DESC_ERR_INVALID, "NULL argument");
    if (m < 0) return fail(DESC_ERR_INVALID, "negative count");
    if (only >= m) return fail(DESC_ERR_INVALID, "only must be an edge or negative");
    if (order)
        for (int64_t e = 0; e < m; ++e) if (order[e] < 0) return fail(DESC_ERR_INVALID, "order holds a negative row");
    DESC_HIP(hipSetDevice(device));
    DevArena A; int rc; double *d_rij, *d_P, *d_einfo; int32_t *d_flags, *d_order = nullptr;
    if ((rc = hook_upload(A, rij, 9 * m, &d_rij)) || (rc = A.alloc(&d_P, (size_t)(9 * m))) || (rc = A.alloc(&d_flags, 2)) || (rc = A.alloc(&d_einfo, 5)) ||
        (order && (rc = hook_upload(A, order, m, &d_order))))
        return rc;
    const int32_t init_flags[2] = {INT_MAX, 0};
    DESC_HIP(hipMemcpy(d_flags, init_flags, sizeof init_flags, hipMemcpyHostToDevice));
    DESC_HIP(hipMemset(d_einfo, 0, sizeof(double) * 5));
    if (m) hipLaunchKernelGGL(k_irls_project, dim3(grid_for(m, 2048)), dim3(256), 0, 0, d_rij, d_order, m, d_P, d_flags, d_flags + 1, (int64_t)-1, d_einfo);
    if (only >= 0) hipLaunchKernelGGL(k_irls_project, dim3(1), dim3(256), 0, 0, d_rij, d_order, m, d_P, d_flags, d_flags + 1, only, d_einfo);
    int32_t flags[2];
    if ((rc = hook_download(flags, d_flags, 2))) return rc;
    *bad_row = flags[0] == INT_MAX ? -1 : flags[0]; *warn = flags[1];
    if ((rc = hook_download(info, d_einfo, 5))) return rc;
    return hook_download(P, d_P, 9 * m);
    });
}

extern "C" int desc_test_irls_node_update(const double* x, const double* Q, int64_t n, int32_t device, double* Q_out, double* score) {
    return no_throw("desc_test_irls_node_update", [&]() -> int {
    if (!x || !Q || !Q_out || !score) return fail(DESC_ERR_INVALID, "NULL argument");
    if (n < 0 || n > INT_MAX) return fail(DESC_ERR_INVALID, "n out of range");
    DESC_HIP(hipSetDevice(device));
    DevArena A; int rc; double *d_x, *d_part; Quat* d_Q;
    const int sgrid = LaaSolver().sgrid;
    if ((rc = hook_upload(A, x, 3 * n, &d_x)) || (rc = hook_upload(A, (const Quat*)Q, n, &d_Q)) || (rc = A.alloc(&d_part, (size_t)sgrid))) return rc;
    hipLaunchKernelGGL(k_l1_node_update, dim3(sgrid), dim3(256), 0, 0, d_x, d_Q, (int)n, d_part);
    hvec<double> part((size_t)sgrid);
    if ((rc = hook_download(part.data(), d_part, sgrid))) return rc;
    double s = 0.0; for (double v : part) s = std::fmax(s, v);
    *score = s;
    return hook_download((Quat*)Q_out, d_Q, n);
    });
}

extern "C" int desc_test_irls_weights(const desc_device_problem* dp, const double* x, const double* B, int64_t m, int32_t mode, double sigma,
                                      double* w) {
    return no_throw("desc_test_irls_weights", [&]() -> int {
    if (!dp || !x || !B || !w) return fail(DESC_ERR_INVALID, "NULL argument");
    if (m < 0 || m != dp->m) return fail(DESC_ERR_INVALID, "m does not match the device problem");
    if (mode != DESC_IRLS_GM && mode != DESC_IRLS_L12) return fail(DESC_ERR_INVALID, "mode must be DESC_IRLS_GM or DESC_IRLS_L12");
    DESC_HIP(hipSetDevice(dp->device));
    DevArena A; int rc; double *d_x, *d_B, *d_w;
    if ((rc = hook_upload(A, x, 3 * dp->n, &d_x)) || (rc = hook_upload(A, B, 3 * m, &d_B)) || (rc = A.alloc(&d_w, (size_t)m))) return rc;
    if (m) hipLaunchKernelGGL(k_irls_weights, dim3(grid_for(m, 2048)), dim3(256), 0, 0, d_x, d_B, dp->d_ii, dp->d_jj, m, mode, sigma, d_w);
    return hook_download(w, d_w, m);
    });
}

// ---- test hooks into the primal-dual solver (tests/test_gpu_pd_kernels.py, tests/test_gpu_pd_solver.py)
// One kernel of pd_solve on a snapshot of the whole state, launched as pd_solve (pd_pcg for gather2) launches it.  edge: the
// PD_EDGE_ARRAYS m x 3 arrays, node: the PD_NODE_ARRAYS n x 3 arrays (the order of pd_arrays), part: the 6 * RG partials; all three are
// uploaded, and come back whole after the launch.
extern "C" int desc_test_irls_pd_stage(const desc_device_problem* dp, int32_t stage, const double* tau, const double* s, const double* ymax,
                                       const int32_t* act, int64_t m, int64_t n, double* edge, double* node, double* part) {
    return no_throw("desc_test_irls_pd_stage", [&]() -> int {
    if (!dp || !tau || !s || !ymax || !act || !edge || !node || !part) return fail(DESC_ERR_INVALID, "NULL argument");
    if (m != dp->m || n != dp->n) return fail(DESC_ERR_INVALID, "m or n does not match the device problem");
    if (stage < 0 || stage >= DESC_TEST_PD_STAGES) return fail(DESC_ERR_INVALID, "unknown stage");
    DESC_HIP(hipSetDevice(dp->device));
    LaaSolver L; PdState S; int rc;
    if ((rc = hook_solver(dp, L)) || (rc = pd_alloc(S, L))) return rc;
    const PdArrays arr = pd_arrays(S);
    for (int k = 0; k < PD_EDGE_ARRAYS; ++k) DESC_HIP(hipMemcpy(*arr.em[k], edge + (size_t)k * 3 * m, sizeof(double) * 3 * m, hipMemcpyHostToDevice));
    for (int k = 0; k < PD_NODE_ARRAYS; ++k) DESC_HIP(hipMemcpy(*arr.nm[k], node + (size_t)k * 3 * n, sizeof(double) * 3 * n, hipMemcpyHostToDevice));
    DESC_HIP(hipMemcpy(S.part, part, sizeof(double) * 6 * RG, hipMemcpyHostToDevice));
    Pd3 a{};
    for (int c = 0; c < 3; ++c) { a.tau[c] = tau[c]; a.s[c] = s[c]; a.ymax[c] = ymax[c]; a.act[c] = act[c] != 0; }
    const int ni = (int)n;
    switch (stage) {
    case DESC_TEST_PD_ABSMAX: hipLaunchKernelGGL(k_pd_absmax, dim3(RG), dim3(256), 0, 0, S.y, m, S.part); break;
    case DESC_TEST_PD_INIT:
        hipLaunchKernelGGL(k_pd_init, dim3(S.egrid), dim3(256), 0, 0, S.y, m, a, S.Ax, S.u, S.f1, S.f2, S.l1, S.l2, S.ev1); break;
    case DESC_TEST_PD_GATHER0:
        hipLaunchKernelGGL(k_pd_gather<0>, dim3(S.rgrid), dim3(256), 0, 0, dp->d_rowptr, dp->d_adj_eid, L.d_sgn, S.ev1, nullptr, a, S.Atv, ni); break;
    case DESC_TEST_PD_GATHER1: {
        Pd3 g = a;
        for (int c = 0; c < 3; ++c) g.tau[c] = pd_gather_coef(a.act[c], a.tau[c]);
        hipLaunchKernelGGL(k_pd_gather<1>, dim3(S.rgrid), dim3(256), 0, 0, dp->d_rowptr, dp->d_adj_eid, L.d_sgn, S.ev1, S.ev2, g, S.w1p, ni);
        break;
    }
    case DESC_TEST_PD_GATHER2: {
        Pd3 none{}; none.act[0] = none.act[1] = none.act[2] = 1;
        hipLaunchKernelGGL(k_pd_gather<2>, dim3(S.rgrid), dim3(256), 0, 0, dp->d_rowptr, dp->d_adj_eid, L.d_sgn, S.sx, nullptr, none, S.dg, ni);
        break;
    }
    case DESC_TEST_PD_PRE:
        hipLaunchKernelGGL(k_pd_pre, dim3(S.egrid), dim3(256), 0, 0, m, a, S.f1, S.f2, S.l1, S.l2, S.w2, S.s1, S.s2, S.sx, S.ev1, S.ev2); break;
    case DESC_TEST_PD_DIR:
        hipLaunchKernelGGL(k_pd_dir, dim3(RG), dim3(256), 0, 0, dp->d_ii, dp->d_jj, m, a, S.dx, S.f1, S.f2, S.l1, S.l2, S.w2, S.s1, S.s2, S.Adx, S.du,
                           S.d1, S.d2, S.ev1, S.part);
        break;
    case DESC_TEST_PD_RESID:
        hipLaunchKernelGGL(k_pd_resid<false>, dim3(RG), dim3(256), 0, 0, m, ni, a, S.y, S.Ax, S.u, S.l1, S.l2, S.Atv, S.Adx, S.du, S.d1, S.d2,
                           S.Atdv, S.part);
        break;
    case DESC_TEST_PD_RESID_TRIAL:
        hipLaunchKernelGGL(k_pd_resid<true>, dim3(RG), dim3(256), 0, 0, m, ni, a, S.y, S.Ax, S.u, S.l1, S.l2, S.Atv, S.Adx, S.du, S.d1, S.d2,
                           S.Atdv, S.part);
        break;
    default:
        hipLaunchKernelGGL(k_pd_accept, dim3(RG), dim3(256), 0, 0, m, ni, a, S.y, S.Ax, S.u, S.l1, S.l2, S.f1, S.f2, S.x, S.Atv, S.dx, S.Adx, S.du,
                           S.d1, S.d2, S.Atdv, S.part);
    }
    for (int k = 0; k < PD_EDGE_ARRAYS; ++k) if ((rc = hook_download(edge + (size_t)k * 3 * m, *arr.em[k], 3 * m))) return rc;
    for (int k = 0; k < PD_NODE_ARRAYS; ++k) if ((rc = hook_download(node + (size_t)k * 3 * n, *arr.nm[k], 3 * n))) return rc;
    return hook_download(part, S.part, 6 * RG);
    });
}

// pd_alloc + pd_solve on B (m x 3) from x = 0.  Out: x (n x 3); state: u, lamu1, lamu2, Ax (m x 3 each) then Atv (n x 3); counters[6]:
// steps, ill, stuck, solves, CG steps, CG solves stopped at the cap; trace: trace_cap records of 3 x 8 doubles (PdTrace), *trace_len
// the number written (the start and every step begun).
extern "C" int desc_test_irls_pd_solve(const desc_device_problem* dp, const double* B, int64_t m, int64_t n, int32_t pdmaxiter, double* x,
                                       double* state, int32_t* counters, double* trace, int32_t trace_cap, int32_t* trace_len) {
    return no_throw("desc_test_irls_pd_solve", [&]() -> int {
    if (!dp || !B || !x || !state || !counters || !trace || !trace_len) return fail(DESC_ERR_INVALID, "NULL argument");
    if (m != dp->m || n != dp->n) return fail(DESC_ERR_INVALID, "m or n does not match the device problem");
    if (pdmaxiter < 0) return fail(DESC_ERR_INVALID, "pdmaxiter must not be negative");
    if (trace_cap < 0) return fail(DESC_ERR_INVALID, "negative trace capacity");
    DESC_HIP(hipSetDevice(dp->device));
    LaaSolver L; PdState S; int rc; double* d_B;
    if ((rc = hook_solver(dp, L)) || (rc = pd_alloc(S, L)) || (rc = hook_upload(L, B, 3 * m, &d_B))) return rc;
    PdTrace tr; tr.rec = trace; tr.cap = trace_cap;
    if ((rc = pd_solve(S, d_B, pdmaxiter, &tr))) return rc;
    *trace_len = tr.len;
    counters[0] = S.steps; counters[1] = S.ill; counters[2] = S.stuck; counters[3] = S.solves; counters[4] = S.cg.total; counters[5] = S.cg.unconverged;
    double* const em[4] = {S.u, S.l1, S.l2, S.Ax};
    for (int k = 0; k < 4; ++k) if ((rc = hook_download(state + (size_t)k * 3 * m, em[k], 3 * m))) return rc;
    if ((rc = hook_download(state + (size_t)12 * m, S.Atv, 3 * n))) return rc;
    return hook_download(x, S.x, 3 * n);
    });
}

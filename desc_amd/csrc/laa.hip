// The Lie-algebraic averaging core (laa.h): Weighted_LAA's step, its PCG, the quantile and the quaternion maps.
//
// Reference text reproduced:
//   Utils/Weighted_LAA.m:4-51      per-edge residual quaternion and log map, weighted least squares
//                                  (W*A) \ (W*B), exp map, quaternion update
//   Utils/Build_Amatrix.m:6-13     incidence matrix with node 1 grounded
//   Utils/R2Q.m:7-14, Utils/q2R.m:1-23
// MATLAB solves the m x (n-1) weighted least-squares problem by sparse QR.  Here the normal
// equations (a grounded graph Laplacian with edge weights w^2, three right-hand sides) are solved
// on the device by Jacobi-preconditioned conjugate gradients in f64 with device-resident scalars
// (no host round trip inside the CG loop); per-edge and per-node maps are plain HIP kernels.
// The primal-dual Newton systems of the IRLS L1 stage (irls.hip) go through the same PCG with one
// weight per edge and coordinate.  `quantile` (Hazen positions, DESC.m:276,301) needs two order
// statistics: a device histogram finds their bins, the host orders the few values in them.
#include <algorithm>
#include <cmath>
#include <vector>

#include "laa.h"

namespace desc {
namespace {

// ---- per-edge / per-node maps ------------------------------------------------------------
__global__ void k_r2q(const double* R, Quat* Q, int64_t count, int transpose) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (int64_t)gridDim.x * blockDim.x) Q[t] = r2q(R + 9 * t, transpose);
}
// q2R.m
__global__ void k_q2r(const Quat* Q, double* R, int64_t n) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        double M[9];
        q2r(Q[t], M);
        for (int k = 0; k < 9; ++k) R[9 * t + k] = M[k];
    }
}

// Weighted_LAA.m:9-37: residual quaternion w = -(conj(Qj) (QQ Qi)), B = log map (3 per edge)
__global__ void k_edge_log(const Quat* Q, const Quat* QQ, const int32_t* ii, const int32_t* jj, double* B, int64_t m) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        double b[3];
        edge_log(QQ[e], Q[ii[e]], Q[jj[e]], b);
        B[3 * e] = b[0]; B[3 * e + 1] = b[1]; B[3 * e + 2] = b[2];
    }
}

// per CSR slot t of node v: neighbour adj[t], edge eid[t], sgn[t] = +1 if v is the edge's j (A has
// +1 in column j, -1 in column i).  16 lanes per node row.
// rhs_v = sum_t sgn * w_e^2 * B_e ;  diag_v = sum_t w_e^2          (normal equations A'W^2A x = A'W^2 B)
__global__ __launch_bounds__(256) void k_rhs(const int32_t* rowptr, const int32_t* eid, const int8_t* sgn, const double* wts,
                                             const double* B, double* rhs, double* diag, int n) {
    const int l16 = threadIdx.x & 15;
    const int row0 = (blockIdx.x * 256 + threadIdx.x) >> 4, nrows = (gridDim.x * 256) >> 4;
    for (int vb = row0 - (row0 % 4); vb < n; vb += nrows) {
        const int v = vb + (row0 % 4);
        double a[3], dg;
        const bool on = v < n;
        rhs_row16(eid, sgn, wts, B, on ? rowptr[v] : 0, on ? rowptr[v + 1] : 0, l16, a, &dg);
        if (v < n && l16 == 0) { rhs[3 * v] = a[0]; rhs[3 * v + 1] = a[1]; rhs[3 * v + 2] = a[2]; diag[v] = dg; }
    }
}

// ---- Jacobi-PCG with device-resident scalars: three right-hand sides share the operator's graph (laa.h: W3, TRACK) -------------
// q_v = sum_t w_e,c (p_v - p_u) for v != 0 (node 0 = MATLAB node 1 is grounded: its unknown is fixed at 0)
template <bool W3>
__global__ __launch_bounds__(256) void k_cg_lap(const int32_t* rowptr, const int32_t* adj, const int32_t* eid, const double* w, const double* p,
                                                double* q, int n) {
    const int l16 = threadIdx.x & 15;
    const int row0 = (blockIdx.x * 256 + threadIdx.x) >> 4, nrows = (gridDim.x * 256) >> 4;
    for (int vb = row0 - (row0 % 4); vb < n; vb += nrows) {
        const int v = vb + (row0 % 4);
        double a[3];
        int t0 = 0, t1 = 0;
        if (v < n && v > 0) { t0 = rowptr[v]; t1 = rowptr[v + 1]; }                     // node 0 is the grounded one: its row stays empty
        lap_row16<W3>(adj, eid, w, p, v, t0, t1, l16, a);
        if (v < n && l16 == 0) { q[3 * v] = a[0]; q[3 * v + 1] = a[1]; q[3 * v + 2] = a[2]; }
    }
}
// one workgroup: column-wise dot products of two n x 3 arrays (fixed order -> reproducible)
__global__ __launch_bounds__(256) void k_cg_dot(const double* a, const double* b, int n, double* out3) {
    double s[3] = {0, 0, 0};
    for (int v = threadIdx.x; v < n; v += 256) for (int c = 0; c < 3; ++c) s[c] += a[3 * v + c] * b[3 * v + c];
    block_reduce<3, 0>(s, out3);
}
// x = 0, r = rhs (node 0 zeroed), z = r/diag, p = z
template <bool W3>
__global__ void k_cg_init(CgScal* sc, const double* rhs, const double* diag, double* x, double* r, double* z, double* p, int n) {
    if (blockIdx.x == 0 && threadIdx.x < 3) sc->bad[threadIdx.x] = 0;
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x)
        for (int c = 0; c < 3; ++c) {
            const double rv = v > 0 ? rhs[3 * v + c] : 0.0;
            const double zv = jacobi<W3>(diag, v, c, rv);
            x[3 * v + c] = 0.0; r[3 * v + c] = rv; z[3 * v + c] = zv; p[3 * v + c] = zv;
        }
}
// alpha = rz/pq (TRACK: 0 once the coordinate broke down) ; x += alpha p ; r -= alpha q ; z = r/diag
template <bool W3, bool TRACK>
__global__ void k_cg_update(CgScal* sc, const double* diag, const double* p, const double* q, double* x, double* r, double* z, int n) {
    double al[3];
    for (int c = 0; c < 3; ++c) {
        const bool brk = TRACK && (sc->bad[c] || cg_breaks(sc->pq[c], sc->rz[c]));
        al[c] = brk ? 0.0 : cg_alpha(sc->rz[c], sc->pq[c]);
    }
    if (TRACK) {
        __syncthreads();
        if (blockIdx.x == 0 && threadIdx.x < 3 && cg_breaks(sc->pq[threadIdx.x], sc->rz[threadIdx.x])) sc->bad[threadIdx.x] = 1;
    }
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x)
        for (int c = 0; c < 3; ++c) {
            const double xv = x[3 * v + c] + al[c] * p[3 * v + c];
            const double rv = r[3 * v + c] - al[c] * q[3 * v + c];
            x[3 * v + c] = xv; r[3 * v + c] = rv;
            z[3 * v + c] = jacobi<W3>(diag, v, c, rv);
        }
}
// beta = rz_new/rz ; p = z + beta p
__global__ void k_cg_dir(const CgScal* sc, const double* z, double* p, int n) {
    double be[3];
    for (int c = 0; c < 3; ++c) be[c] = cg_beta(sc->rz[c], sc->rz_new[c]);
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x)
        for (int c = 0; c < 3; ++c) p[3 * v + c] = z[3 * v + c] + be[c] * p[3 * v + c];
}
// rz = rz_new
template <bool TRACK>
__global__ void k_cg_roll(CgScal* sc) {
    if (threadIdx.x < 3) {
        if (TRACK && !isfinite(sc->rz_new[threadIdx.x])) sc->bad[threadIdx.x] = 1;
        sc->rz[threadIdx.x] = sc->rz_new[threadIdx.x];
    }
}

// Weighted_LAA.m:40-50: score, exp map, Q <- Q * W ; x holds the tangent solution (row 0 = 0)
__global__ __launch_bounds__(256) void k_node_update(const double* x, Quat* Q, double* Wv /* n x 3: vector part of the quaternion W */,
                                                     int n, double* score_partial) {
    double sc = 0.0;
    for (int v = blockIdx.x * 256 + threadIdx.x; v < n; v += gridDim.x * 256) {
        const double theta = node_update(x + 3 * v, Q + v, Wv + 3 * v);          // :42-46
        if (v > 0) sc += theta;                                                       // :40 (rows 2:end)
    }
    __shared__ double sh[4];
    const double tot = score_chunk_sum(sc, sh);
    if (threadIdx.x == 0) score_partial[blockIdx.x] = tot;
}
// DESC.m:298-303
__global__ void k_weights(const double* RS, double* wts, int64_t m, double thresh, double wmax, double wmin) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        wts[e] = laa_weight(RS[e], thresh, wmax, wmin);
    }
}

// ---- MATLAB's quantile on the device: a 4096-bin histogram over [lo, hi] locates the two order statistics the Hazen
// interpolation needs, the values of their bins (a few hundred of m) are collected and ordered on the host.
constexpr int QBINS = 4096;
__device__ __forceinline__ int qbin(double x, double lo, double scale) {
    const int b = (int)((x - lo) * scale);
    return b < 0 ? 0 : (b >= QBINS ? QBINS - 1 : b);
}
__global__ __launch_bounds__(256) void k_minmax(const double* x, int64_t m, double* out /* [grid][2] */) {
    double lo[1] = {INFINITY}, hi[1] = {-INFINITY};
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256) { lo[0] = fmin(lo[0], x[e]); hi[0] = fmax(hi[0], x[e]); }
    block_reduce<1, 1>(lo, out + 2 * blockIdx.x);
    block_reduce<1, 2>(hi, out + 2 * blockIdx.x + 1);
}
__global__ __launch_bounds__(256) void k_qhist(const double* x, int64_t m, double lo, double scale, unsigned* hist) {
    __shared__ unsigned h[QBINS];
    for (int t = threadIdx.x; t < QBINS; t += 256) h[t] = 0;
    __syncthreads();
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256) atomicAdd(&h[qbin(x[e], lo, scale)], 1u);
    __syncthreads();
    for (int t = threadIdx.x; t < QBINS; t += 256) if (h[t]) atomicAdd(&hist[t], h[t]);
}
__global__ __launch_bounds__(256) void k_qcollect(const double* x, int64_t m, double lo, double scale, int b0, int b1, double* out, unsigned* count, unsigned cap) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256) {
        const int b = qbin(x[e], lo, scale);
        if (b == b0 || b == b1) { const unsigned p = atomicAdd(count, 1u); if (p < cap) out[p] = x[e]; }
    }
}

// MATLAB quantile(x, p): Hazen plotting positions (k-0.5)/n, linear interpolation, clamped
double matlab_quantile(hvec<double>& x, double p) {
    const size_t n = x.size();
    if (n == 0) return NAN;
    int64_t k0 = 0; double fr = 0.0;
    const int where = hazen_position((int64_t)n, p, &k0, &fr);
    if (where == HAZEN_MIN) return *std::min_element(x.begin(), x.end());
    if (where == HAZEN_MAX) return *std::max_element(x.begin(), x.end());
    const size_t lo = (size_t)k0;                        // 0-based
    std::nth_element(x.begin(), x.begin() + lo, x.end());
    const double a = x[lo];
    const double b = *std::min_element(x.begin() + lo + 1, x.end());
    return hazen_interp(a, b, fr);
}

// quantile(x, p) of a device vector, MATLAB's definition (the same order statistics as matlab_quantile above);
// scratch: d_mm [64][2] doubles, d_hist QBINS unsigned + 1 counter, d_cand cap doubles
int device_quantile(const double* d_x, int64_t m, double p, double* d_mm, unsigned* d_hist, double* d_cand, unsigned cap, double* result) {
    if (m == 0) { *result = NAN; return DESC_OK; }
    const int g = grid_for(m, 1024);
    hipLaunchKernelGGL(k_minmax, dim3(64), dim3(256), 0, 0, d_x, m, d_mm);
    double mm[128];
    DESC_HIP(hipMemcpy(mm, d_mm, sizeof mm, hipMemcpyDeviceToHost));
    double lo = INFINITY, hi = -INFINITY;
    for (int b = 0; b < 64; ++b) { lo = std::min(lo, mm[2 * b]); hi = std::max(hi, mm[2 * b + 1]); }
    int64_t k0 = 0; double fr = 0.0;                        // 0-based rank of the lower order statistic; the upper one is k0 + 1
    const int where = hazen_position(m, p, &k0, &fr);
    if (where == HAZEN_MIN) { *result = lo; return DESC_OK; }
    if (where == HAZEN_MAX) { *result = hi; return DESC_OK; }
    if (hazen_flat(lo, hi)) { *result = lo; return DESC_OK; }
    const double scale = (double)QBINS / (hi - lo) * (1.0 - 1e-12);
    DESC_HIP(hipMemset(d_hist, 0, sizeof(unsigned) * (QBINS + 1)));
    hipLaunchKernelGGL(k_qhist, dim3(g), dim3(256), 0, 0, d_x, m, lo, scale, d_hist);
    hvec<unsigned> hist(QBINS);
    DESC_HIP(hipMemcpy(hist.data(), d_hist, sizeof(unsigned) * QBINS, hipMemcpyDeviceToHost));
    int64_t acc = 0; int b0 = -1, b1 = -1; int64_t base0 = 0;
    for (int b = 0; b < QBINS; ++b) {
        if (b0 < 0 && acc + hist[b] > (uint64_t)k0) { b0 = b; base0 = acc; }
        if (b0 >= 0 && acc + hist[b] > (uint64_t)(k0 + 1)) { b1 = b; break; }
        acc += hist[b];
    }
    if (b0 < 0 || b1 < 0) return fail(DESC_ERR_STATE, "quantile histogram inconsistent");
    const uint64_t need = (uint64_t)hist[b0] + (b1 != b0 ? hist[b1] : 0);
    if (need > cap) {                                       // a bin too full to collect (heavily tied data): exact host path
        hvec<double> all((size_t)m);
        DESC_HIP(hipMemcpy(all.data(), d_x, sizeof(double) * m, hipMemcpyDeviceToHost));
        *result = matlab_quantile(all, p);
        return DESC_OK;
    }
    hipLaunchKernelGGL(k_qcollect, dim3(g), dim3(256), 0, 0, d_x, m, lo, scale, b0, b1, d_cand, d_hist + QBINS, cap);
    hvec<double> cand((size_t)need);
    DESC_HIP(hipMemcpy(cand.data(), d_cand, sizeof(double) * need, hipMemcpyDeviceToHost));
    std::sort(cand.begin(), cand.end());
    // cand = bin b0 (ranks base0 ...) followed, if different, by bin b1 (which starts at rank >= k0 + 1)
    const double a = cand[(size_t)(k0 - base0)];
    const double bnext = (b1 == b0) ? cand[(size_t)(k0 + 1 - base0)] : cand[(size_t)hist[b0] + 0 + (size_t)0];
    *result = hazen_interp(a, bnext, fr);
    return DESC_OK;
}

// Build_Amatrix.m:10: -1 at the smaller endpoint i, +1 at j -- per CSR slot
__global__ void k_incidence_sign(const int32_t* rowptr, const int32_t* adj, int8_t* sgn, int n) {
    const int l16 = threadIdx.x & 15;
    const int row0 = (blockIdx.x * 256 + threadIdx.x) >> 4, nrows = (gridDim.x * 256) >> 4;
    for (int v = row0; v < n; v += nrows)
        for (int t = rowptr[v] + l16; t < rowptr[v + 1]; t += 16) sgn[t] = v < adj[t] ? -1 : +1;
}

constexpr unsigned QCAP = 1u << 20;     // most values device_quantile collects from the two bins

}  // namespace

int laa_setup(const desc_device_problem* dp, const double* R_init, LaaSolver& L) {
    int rc = DESC_OK;
    const int64_t n = dp->n, m = dp->m;
    L.dp = dp; L.n = n; L.m = m;
    if ((rc = L.alloc(&L.d_sgn, 2 * m)) || (rc = L.alloc(&L.d_Rinit, 9 * n)) || (rc = L.alloc(&L.d_w, m)) || (rc = L.alloc(&L.d_B, 3 * m)) ||
        (rc = L.alloc(&L.d_rhs, 3 * n)) || (rc = L.alloc(&L.d_diag, n)) || (rc = L.alloc(&L.d_x, 3 * n)) || (rc = L.alloc(&L.d_r, 3 * n)) ||
        (rc = L.alloc(&L.d_z, 3 * n)) || (rc = L.alloc(&L.d_p, 3 * n)) || (rc = L.alloc(&L.d_q, 3 * n)) || (rc = L.alloc(&L.d_Wv, 3 * n)) ||
        (rc = L.alloc(&L.d_score, L.sgrid)) || (rc = L.alloc(&L.d_Rout, 9 * n)) || (rc = L.alloc(&L.d_Q, n)) || (rc = L.alloc(&L.d_QQ, m)) ||
        (rc = L.alloc(&L.d_sc, 1)))
        return rc;
    if ((rc = L.alloc(&L.d_mm, 128)) || (rc = L.alloc(&L.d_cand, QCAP)) || (rc = L.alloc(&L.d_qh, QBINS + 1))) return rc;
    L.part.resize(L.sgrid);
    DESC_HIP(hipMemcpy(L.d_Rinit, R_init, sizeof(double) * 9 * n, hipMemcpyHostToDevice));
    L.egrid = grid_for(m, 2048);
    L.ngrid = grid_for(n, 512);
    L.rgrid = grid_for(n * 16, 2048);
    if (m) hipLaunchKernelGGL(k_incidence_sign, dim3(L.rgrid), dim3(256), 0, 0, dp->d_rowptr, dp->d_adj, L.d_sgn, (int)n);
    hipLaunchKernelGGL(k_r2q, dim3(L.ngrid), dim3(256), 0, 0, L.d_Rinit, L.d_Q, n, 0);              // Q = R2Q(R_init)        (DESC.m:270, MPLS.m:205)
    if (m) hipLaunchKernelGGL(k_r2q, dim3(L.egrid), dim3(256), 0, 0, dp->d_rij, L.d_QQ, m, 1);      // QQ = R2Q(permute(RijMat)) (:265,271; MPLS.m:200,206)
    return DESC_OK;
}

template <bool W3, bool TRACK>
int laa_pcg(LaaSolver& L, const double* w, const double* rhs, const double* diag, double* x, const int act[3], int probe, CgCount& count, int bad[3]) {
    const desc_device_problem* dp = L.dp;
    const int n = (int)L.n, ngrid = L.ngrid, rgrid = L.rgrid;
    CgScal* sc = L.d_sc;
    auto dot = [&](const double* a, const double* b, double* out3) { hipLaunchKernelGGL(k_cg_dot, dim3(1), dim3(256), 0, 0, a, b, n, out3); };
    hipLaunchKernelGGL(k_cg_init<W3>, dim3(ngrid), dim3(256), 0, 0, sc, rhs, diag, x, L.d_r, L.d_z, L.d_p, n);
    dot(L.d_r, L.d_z, sc->rz);
    dot(L.d_r, L.d_r, sc->bnorm);
    const int cg_max = (int)std::min<int64_t>(20000, 20 * L.n + 200);
    CgScal hs;
    bool done = false;
    int k = 0;
    for (k = 1; k <= cg_max; ++k) {
        hipLaunchKernelGGL(k_cg_lap<W3>, dim3(rgrid), dim3(256), 0, 0, dp->d_rowptr, dp->d_adj, dp->d_adj_eid, w, L.d_p, L.d_q, n);
        dot(L.d_p, L.d_q, sc->pq);
        hipLaunchKernelGGL((k_cg_update<W3, TRACK>), dim3(ngrid), dim3(256), 0, 0, sc, diag, L.d_p, L.d_q, x, L.d_r, L.d_z, n);
        dot(L.d_r, L.d_z, sc->rz_new);
        hipLaunchKernelGGL(k_cg_dir, dim3(ngrid), dim3(256), 0, 0, sc, L.d_z, L.d_p, n);
        hipLaunchKernelGGL(k_cg_roll<TRACK>, dim3(1), dim3(64), 0, 0, sc);
        if (k % probe == 0 || k == cg_max) {                                               // convergence probe: |r| <= 1e-13 |b|
            dot(L.d_r, L.d_r, sc->rnorm);
            DESC_HIP(hipMemcpy(&hs, sc, sizeof hs, hipMemcpyDeviceToHost));
            done = true;
            for (int c = 0; c < 3; ++c)
                if (act[c] && !hs.bad[c] && cg_unfinished(hs.rnorm[c], hs.bnorm[c])) done = false;
            if (done || k == cg_max) break;
        }
    }
    count.total += std::min(k, cg_max);                                                    // the true count rounded up to the probe interval
    for (int c = 0; c < 3; ++c) {
        bad[c] = act[c] && hs.bad[c];
        if (act[c] && !bad[c] && hs.bnorm[c] > 0) count.worst = std::max(count.worst, std::sqrt(hs.rnorm[c] / hs.bnorm[c]));
    }
    if (!done) ++count.unconverged;
    return DESC_OK;
}
template int laa_pcg<false, false>(LaaSolver&, const double*, const double*, const double*, double*, const int*, int, CgCount&, int*);
template int laa_pcg<true, true>(LaaSolver&, const double*, const double*, const double*, double*, const int*, int, CgCount&, int*);

int laa_step(LaaSolver& L, double* score_out) {
    const desc_device_problem* dp = L.dp;
    const int64_t n = L.n;
    int rc = DESC_OK;
    laa_edge_log(L);
    hipLaunchKernelGGL(k_rhs, dim3(L.rgrid), dim3(256), 0, 0, dp->d_rowptr, dp->d_adj_eid, L.d_sgn, L.d_w, L.d_B, L.d_rhs, L.d_diag, (int)n);
    const int all[3] = {1, 1, 1};
    int bad[3];
    if ((rc = laa_pcg<false, false>(L, L.d_w, L.d_rhs, L.d_diag, L.d_x, all, 25, L.cg, bad))) return rc;
    hipLaunchKernelGGL(k_node_update, dim3(L.sgrid), dim3(256), 0, 0, L.d_x, L.d_Q, L.d_Wv, (int)n, L.d_score);
    DESC_HIP(hipMemcpy(L.part.data(), L.d_score, sizeof(double) * L.sgrid, hipMemcpyDeviceToHost));
    double score = 0.0; for (double v : L.part) score += v;
    *score_out = score / (double)n;                                                     // Weighted_LAA.m:40
    return DESC_OK;
}

void laa_set_qq(LaaSolver& L, const double* d_blocks) {
    if (L.m) hipLaunchKernelGGL(k_r2q, dim3(L.egrid), dim3(256), 0, 0, d_blocks, L.d_QQ, L.m, 0);
}

void laa_edge_log(LaaSolver& L) {
    if (L.m) hipLaunchKernelGGL(k_edge_log, dim3(L.egrid), dim3(256), 0, 0, L.d_Q, L.d_QQ, L.dp->d_ii, L.dp->d_jj, L.d_B, L.m);
}

void laa_weights(LaaSolver& L, const double* d_x, double thresh) {
    if (L.m) hipLaunchKernelGGL(k_weights, dim3(L.egrid), dim3(256), 0, 0, d_x, L.d_w, L.m, thresh, 1e4, 1e-4);    // DESC.m:280-281, MPLS.m:211-212
}

int laa_quantile(LaaSolver& L, const double* d_x, double p, double* result) {
    return device_quantile(d_x, L.m, p, L.d_mm, L.d_qh, L.d_cand, QCAP, result);
}

int laa_finish(LaaSolver& L, int iterations, double* R_out) {
    if (L.cg.unconverged)
        fprintf(stderr, "[desc_amd] warning: %d of %d Weighted_LAA solves stopped at the PCG iteration cap (relative residual up to %.3e)\n",
                L.cg.unconverged, iterations, L.cg.worst);
    hipLaunchKernelGGL(k_q2r, dim3(L.ngrid), dim3(256), 0, 0, L.d_Q, L.d_Rout, L.n);                // DESC.m:309-312, MPLS.m:251-254
    DESC_HIP(hipDeviceSynchronize());
    DESC_HIP(hipMemcpy(R_out, L.d_Rout, sizeof(double) * 9 * L.n, hipMemcpyDeviceToHost));
    return DESC_OK;
}

}  // namespace desc

// ---- test hooks (include/desc_amd.h, tests/test_gpu_laa_maps.py): one operation of the core on caller (host) arrays, with the kernel
// and the grid rule of the product path (laa_setup's egrid / ngrid / rgrid / sgrid).  Nothing in the library calls them.
using namespace desc;

namespace desc {

// the solver state of laa_setup on dp (identity R_init): grids, incidence signs, work arrays
int hook_solver(const desc_device_problem* dp, LaaSolver& L) {
    if (dp->m && !dp->d_rij) return fail(DESC_ERR_INVALID, "the device problem holds no rotations");
    hvec<double> eye((size_t)9 * dp->n, 0.0);
    for (int64_t v = 0; v < dp->n; ++v) eye[9 * v] = eye[9 * v + 4] = eye[9 * v + 8] = 1.0;
    return laa_setup(dp, eye.data(), L);
}

}  // namespace desc

extern "C" int desc_test_laa_r2q(const double* R, int64_t count, int32_t transpose, int32_t edge_grid, int32_t device, double* Q) {
    return no_throw("desc_test_laa_r2q", [&]() -> int {
    if (!R || !Q) return fail(DESC_ERR_INVALID, "NULL argument");
    if (count < 0) return fail(DESC_ERR_INVALID, "negative count");
    DESC_HIP(hipSetDevice(device));
    DevArena A; int rc; double* d_R; Quat* d_Q;
    if ((rc = hook_upload(A, R, 9 * count, &d_R)) || (rc = A.alloc(&d_Q, (size_t)count))) return rc;
    const int grid = edge_grid ? grid_for(count, 2048) : grid_for(count, 512);                       // laa_setup: egrid / ngrid
    if (count) hipLaunchKernelGGL(k_r2q, dim3(grid), dim3(256), 0, 0, d_R, d_Q, count, transpose ? 1 : 0);
    return hook_download((Quat*)Q, d_Q, count);
    });
}

extern "C" int desc_test_laa_q2r(const double* Q, int64_t n, int32_t device, double* R) {
    return no_throw("desc_test_laa_q2r", [&]() -> int {
    if (!Q || !R) return fail(DESC_ERR_INVALID, "NULL argument");
    if (n < 0) return fail(DESC_ERR_INVALID, "negative count");
    DESC_HIP(hipSetDevice(device));
    DevArena A; int rc; Quat* d_Q; double* d_R;
    if ((rc = hook_upload(A, (const Quat*)Q, n, &d_Q)) || (rc = A.alloc(&d_R, (size_t)(9 * n)))) return rc;
    if (n) hipLaunchKernelGGL(k_q2r, dim3(grid_for(n, 512)), dim3(256), 0, 0, d_Q, d_R, n);          // laa_finish
    return hook_download(R, d_R, 9 * n);
    });
}

extern "C" int desc_test_laa_edge_log(const desc_device_problem* dp, const double* Q, const double* QQ, int64_t m, double* B) {
    return no_throw("desc_test_laa_edge_log", [&]() -> int {
    if (!dp || !Q || !QQ || !B) return fail(DESC_ERR_INVALID, "NULL argument");
    if (m < 0 || m != dp->m) return fail(DESC_ERR_INVALID, "m does not match the device problem");
    DESC_HIP(hipSetDevice(dp->device));
    LaaSolver L; int rc;
    if ((rc = hook_solver(dp, L))) return rc;
    DESC_HIP(hipMemcpy(L.d_Q, Q, sizeof(Quat) * L.n, hipMemcpyHostToDevice));
    if (m) DESC_HIP(hipMemcpy(L.d_QQ, QQ, sizeof(Quat) * m, hipMemcpyHostToDevice));
    laa_edge_log(L);
    return hook_download(B, L.d_B, 3 * m);
    });
}

extern "C" int desc_test_laa_rhs(const desc_device_problem* dp, const double* w, const double* B, int64_t m, double* rhs, double* diag) {
    return no_throw("desc_test_laa_rhs", [&]() -> int {
    if (!dp || !w || !B || !rhs || !diag) return fail(DESC_ERR_INVALID, "NULL argument");
    if (m < 0 || m != dp->m) return fail(DESC_ERR_INVALID, "m does not match the device problem");
    DESC_HIP(hipSetDevice(dp->device));
    LaaSolver L; int rc;
    if ((rc = hook_solver(dp, L))) return rc;
    if (m) { DESC_HIP(hipMemcpy(L.d_w, w, sizeof(double) * m, hipMemcpyHostToDevice)); DESC_HIP(hipMemcpy(L.d_B, B, sizeof(double) * 3 * m, hipMemcpyHostToDevice)); }
    hipLaunchKernelGGL(k_rhs, dim3(L.rgrid), dim3(256), 0, 0, dp->d_rowptr, dp->d_adj_eid, L.d_sgn, L.d_w, L.d_B, L.d_rhs, L.d_diag, (int)L.n);   // laa_step
    if ((rc = hook_download(rhs, L.d_rhs, 3 * L.n))) return rc;
    return hook_download(diag, L.d_diag, L.n);
    });
}

extern "C" int desc_test_laa_pcg(const desc_device_problem* dp, int32_t w3, const double* w, const double* rhs, const double* diag, int64_t m,
                                 const int32_t* act, double* x, int32_t* bad, double* rnorm, double* bnorm, int32_t* total,
                                 int32_t* unconverged, double* worst) {
    return no_throw("desc_test_laa_pcg", [&]() -> int {
    if (!dp || !w || !rhs || !diag || !act || !x || !bad || !rnorm || !bnorm || !total || !unconverged || !worst)
        return fail(DESC_ERR_INVALID, "NULL argument");
    if (m < 0 || m != dp->m) return fail(DESC_ERR_INVALID, "m does not match the device problem");
    DESC_HIP(hipSetDevice(dp->device));
    LaaSolver L; int rc;
    if ((rc = hook_solver(dp, L))) return rc;
    const int64_t n = L.n, wlen = w3 ? 3 * m : m, dlen = w3 ? 3 * n : n;
    double *d_w, *d_diag, *d_xx;
    if ((rc = hook_upload<double>(L, w, wlen, &d_w)) || (rc = hook_upload<double>(L, diag, dlen, &d_diag)) || (rc = L.alloc(&d_xx, (size_t)(3 * n)))) return rc;
    DESC_HIP(hipMemcpy(L.d_rhs, rhs, sizeof(double) * 3 * n, hipMemcpyHostToDevice));
    const int a3[3] = {act[0] != 0, act[1] != 0, act[2] != 0};
    int b3[3] = {0, 0, 0};
    CgCount cnt;
    rc = w3 ? laa_pcg<true, true>(L, d_w, L.d_rhs, d_diag, d_xx, a3, 5, cnt, b3)                   // pd_pcg (irls.hip): PD_PROBE
            : laa_pcg<false, false>(L, d_w, L.d_rhs, d_diag, d_xx, a3, 25, cnt, b3);               // laa_step
    if (rc) return rc;
    CgScal hs;
    if ((rc = hook_download(&hs, L.d_sc, 1))) return rc;
    for (int c = 0; c < 3; ++c) { bad[c] = b3[c]; rnorm[c] = hs.rnorm[c]; bnorm[c] = hs.bnorm[c]; }
    *total = cnt.total; *unconverged = cnt.unconverged; *worst = cnt.worst;
    return hook_download(x, d_xx, 3 * n);
    });
}

extern "C" int desc_test_laa_node_update(const double* x, const double* Q, int64_t n, int32_t device, double* Q_out, double* Wv, double* score) {
    return no_throw("desc_test_laa_node_update", [&]() -> int {
    if (!x || !Q || !Q_out || !Wv || !score) return fail(DESC_ERR_INVALID, "NULL argument");
    if (n < 0 || n > INT32_MAX) return fail(DESC_ERR_INVALID, "n out of range");
    DESC_HIP(hipSetDevice(device));
    DevArena A; int rc; double *d_x, *d_Wv, *d_part; Quat* d_Q;
    const int sgrid = LaaSolver().sgrid;
    if ((rc = hook_upload(A, x, 3 * n, &d_x)) || (rc = hook_upload(A, (const Quat*)Q, n, &d_Q)) || (rc = A.alloc(&d_Wv, (size_t)(3 * n))) ||
        (rc = A.alloc(&d_part, (size_t)sgrid)))
        return rc;
    hipLaunchKernelGGL(k_node_update, dim3(sgrid), dim3(256), 0, 0, d_x, d_Q, d_Wv, (int)n, d_part);   // laa_step
    hvec<double> part((size_t)sgrid);
    if ((rc = hook_download(part.data(), d_part, sgrid))) return rc;
    double s = 0.0; for (double v : part) s += v;
    *score = s;                                                                                      // laa_step divides this by n
    if ((rc = hook_download((Quat*)Q_out, d_Q, n))) return rc;
    return hook_download(Wv, d_Wv, 3 * n);
    });
}

extern "C" int desc_test_laa_weights(const double* x, int64_t m, double thresh, int32_t device, double* w) {
    return no_throw("desc_test_laa_weights", [&]() -> int {
    if (!x || !w) return fail(DESC_ERR_INVALID, "NULL argument");
    if (m < 0) return fail(DESC_ERR_INVALID, "negative count");
    DESC_HIP(hipSetDevice(device));
    DevArena A; int rc; double *d_x, *d_w;
    if ((rc = hook_upload(A, x, m, &d_x)) || (rc = A.alloc(&d_w, (size_t)m))) return rc;
    if (m) hipLaunchKernelGGL(k_weights, dim3(grid_for(m, 2048)), dim3(256), 0, 0, d_x, d_w, m, thresh, 1e4, 1e-4);   // laa_weights
    return hook_download(w, d_w, m);
    });
}

extern "C" int desc_test_laa_quantile(const double* x, int64_t m, double p, int64_t cap, int32_t device, double* result) {
    return no_throw("desc_test_laa_quantile", [&]() -> int {
    if (!x || !result) return fail(DESC_ERR_INVALID, "NULL argument");
    if (m < 0) return fail(DESC_ERR_INVALID, "negative count");
    if (!(p >= 0.0 && p <= 1.0)) return fail(DESC_ERR_INVALID, "p must lie in [0, 1]");
    if (cap < 1 || cap > (int64_t)QCAP) return fail(DESC_ERR_INVALID, "cap must lie in [1, %u]", QCAP);
    DESC_HIP(hipSetDevice(device));
    DevArena A; int rc; double *d_x, *d_mm, *d_cand; unsigned* d_qh;
    if ((rc = hook_upload(A, x, m, &d_x)) || (rc = A.alloc(&d_mm, 128)) || (rc = A.alloc(&d_cand, (size_t)cap)) || (rc = A.alloc(&d_qh, QBINS + 1))) return rc;
    return device_quantile(d_x, m, p, d_mm, d_qh, d_cand, (unsigned)cap, result);
    });
}

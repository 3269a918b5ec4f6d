// The Weighted-LAA loop of ONE problem inside ONE workgroup of 256 threads, shared by k_refine_batch (refine_batch.hip), k_mpls_batch
// (mpls_batch.hip) and k_irls_batch (irls_batch.hip): one text, so a problem gets the same bits whichever of them steps it (as laa_math.h, cemp_math.h and small_dense.h
// for their callers).
//   WgLaa / wg_laa_views   the per-node state in dynamic LDS, 26 doubles per node (Q; x r z p q rhs; diag; Wv), addressed with the
//                          problem's own n, and the problem's views of the per-edge arrays in global memory
//   wg_pcg<W3, TRACK>      laa_pcg of laa.h: the Jacobi-PCG of three right-hand sides with its probe; <true, true> serves the primal-dual
//                          Newton systems of k_irls_batch (irls_batch.hip)
//   wg_laa_step            Weighted_LAA.m: the edge log map, the normal equations, wg_pcg<false, false> with its probe every 25 steps,
//                          the exp map, Q <- Q * W, the score in chunks of 256 rows
//   wg_quantile            MATLAB's quantile of a per-edge array: the extrema, the Hazen position, the two order statistics by an exact
//                          radix select over the 64-bit order key (8-bit digits, integer histogram in LDS), their interpolation
//   wg_select              that radix select alone: the order statistics of two neighbouring ranks (also the median of align_batch.hip)
// Reductions keep the single path's orders: a CSR row by the 16 lanes of a DPP row (rhs_row16 / lap_row16), the PCG's dot products by
// k_cg_dot's loop and block_reduce<3, 0>, the score by score_chunk_sum added in ascending order from 0.0.
//
// Control flow.  Every thread of the workgroup calls these functions together.  Every decision around a barrier is taken by every
// thread from the same LDS values with the same instructions, and the integers that steer loops and barriers go through readfirstlane.
// Every loop is bounded by cg_max, a row length, m or the 8 digit passes.  No spinning on memory, no floating-point atomic.
#pragma once
#include <cmath>

#include "laa_math.h"
#include "mst_key.h"

namespace desc {

constexpr int RB_LDS_BYTES = 160 * 1024;               // what one workgroup may declare on gfx950
constexpr int RB_NODE_DOUBLES = 4 + 6 * 3 + 1 + 3;     // Q; x r z p q rhs; diag; Wv
constexpr int RB_STATIC_BYTES = 8 * 1024;              // set aside for the kernel's fixed LDS: block_reduce's tree (6 KiB), the histogram (1 KiB), scalars
constexpr int REFINE_BATCH_MAX_N = (RB_LDS_BYTES - RB_STATIC_BYTES) / (8 * RB_NODE_DOUBLES);    // 748
static_assert(REFINE_BATCH_MAX_N >= 278, "the cap of DESC_batch is the eigen-solve's");
constexpr int RB_PROBE = 25;                           // laa_step's probe interval

inline size_t rb_lds_bytes(int n) { return sizeof(double) * (size_t)RB_NODE_DOUBLES * (size_t)n; }

// one problem as its workgroup sees it
struct WgLaa {
    int n, m;
    const int32_t *rowptr, *adj, *eid;                  // the problem's CSR, local ids
    const int8_t* sgn;                                  // incidence sign per CSR slot
    const int32_t *ii, *jj;                             // local endpoints
    Quat* QQ;                                           // m, global
    double *B, *w;                                      // 3 m, m, global
    Quat* Q;                                            // LDS from here on
    double *x, *r, *z, *p, *q, *rhs, *diag, *Wv;
};
// the PCG's bookkeeping over the steps of a run (LaaSolver::cg)
struct WgCg { int total = 0, unconverged = 0; double worst_sq = 0.0; };

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double key_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

__device__ __forceinline__ void wg_laa_views(double* lds, int n, WgLaa& s) {
    s.Q = (Quat*)lds;
    s.x = lds + 4 * n;
    s.r = s.x + 3 * n;
    s.z = s.r + 3 * n;
    s.p = s.z + 3 * n;
    s.q = s.p + 3 * n;
    s.rhs = s.q + 3 * n;
    s.diag = s.rhs + 3 * n;
    s.Wv = s.diag + n;
}

// k_cg_dot in place: column-wise dot products of two n x 3 arrays into out3 (LDS).  Ends with a barrier.
__device__ __forceinline__ void rb_dot(const double* a, const double* b, int n, double* out3) {
    double s[3] = {0, 0, 0};
    for (int v = threadIdx.x; v < n; v += 256) for (int c = 0; c < 3; ++c) s[c] += a[3 * v + c] * b[3 * v + c];
    block_reduce<3, 0>(s, out3);
    __syncthreads();
}

// laa_pcg<W3, TRACK> (laa.h) inside the workgroup: x_c = (A' diag(w_c) A) \ rhs_c for the three coordinates, x r z p q rhs diag in LDS,
// the weights in global memory (W3: w[3 e + c] and diag[3 v + c], else w[e] * w[e] and diag[v]), the probe |r| <= 1e-13 |b| every `probe`
// steps over the coordinates in act.  TRACK: a breakdown freezes its coordinate, takes it out of the probe and comes back in
// bad_out[c]; else bad_out[] comes back 0.  The bookkeeping of the solve is added to cg.  Expects a barrier behind the last write of
// rhs, diag and w; ends with one.
template <bool W3, bool TRACK>
__device__ __forceinline__ void wg_pcg(int n, const int32_t* rowptr, const int32_t* adj, const int32_t* eid, const double* w, const double* rhs,
                                       const double* diag, double* x, double* r, double* z, double* p, double* q, const int act[3], int probe,
                                       int cg_max, WgCg& cg, int bad_out[3]) {
    __shared__ double cgs[15];                          // rz, rz_new, pq, bnorm, rnorm: CgScal's doubles
    __shared__ int cg_bad[3];                           // CgScal's bad
    const int tid = threadIdx.x, l16 = tid & 15, row = tid >> 4;
    double *rz = cgs, *rz_new = cgs + 3, *pq = cgs + 6, *bnorm = cgs + 9, *rnorm = cgs + 12;
    // ---- x = 0, r = rhs (node 0 zeroed), z = r / diag, p = z
    if (TRACK && tid < 3) cg_bad[tid] = 0;
    for (int v = tid; v < n; v += 256)
        for (int c = 0; c < 3; ++c) {
            const double rv = v > 0 ? rhs[3 * v + c] : 0.0;
            const double zv = jacobi<W3>(diag, v, c, rv);
            x[3 * v + c] = 0.0; r[3 * v + c] = rv; z[3 * v + c] = zv; p[3 * v + c] = zv;
        }
    __syncthreads();
    rb_dot(r, z, n, rz);
    rb_dot(r, r, n, bnorm);
    int done = 0, k = 0;
    for (k = 1; k <= cg_max; ++k) {
        for (int vb = 0; vb < n; vb += 16) {
            const int v = vb + row;
            const bool on = v < n && v > 0;
            double s3[3];
            lap_row16<W3>(adj, eid, w, p, v, on ? rowptr[v] : 0, on ? rowptr[v + 1] : 0, l16, s3);
            if (v < n && l16 == 0) { q[3 * v] = s3[0]; q[3 * v + 1] = s3[1]; q[3 * v + 2] = s3[2]; }
        }
        __syncthreads();
        rb_dot(p, q, n, pq);
        double al[3];
        for (int c = 0; c < 3; ++c) {
            const bool brk = TRACK && (cg_bad[c] || cg_breaks(pq[c], rz[c]));
            al[c] = brk ? 0.0 : cg_alpha(rz[c], pq[c]);
        }
        if (TRACK) {
            __syncthreads();                                                            // every thread has read cg_bad
            if (tid < 3 && cg_breaks(pq[tid], rz[tid])) cg_bad[tid] = 1;
        }
        for (int v = tid; v < n; v += 256)
            for (int c = 0; c < 3; ++c) {
                const double xv = x[3 * v + c] + al[c] * p[3 * v + c];
                const double rv = r[3 * v + c] - al[c] * q[3 * v + c];
                x[3 * v + c] = xv; r[3 * v + c] = rv;
                z[3 * v + c] = jacobi<W3>(diag, v, c, rv);
            }
        __syncthreads();
        rb_dot(r, z, n, rz_new);
        double be[3];
        for (int c = 0; c < 3; ++c) be[c] = cg_beta(rz[c], rz_new[c]);
        for (int v = tid; v < n; v += 256)
            for (int c = 0; c < 3; ++c) p[3 * v + c] = z[3 * v + c] + be[c] * p[3 * v + c];
        __syncthreads();                                                                // every thread has read rz
        if (tid < 3) {
            if (TRACK && !isfinite(rz_new[tid])) cg_bad[tid] = 1;
            rz[tid] = rz_new[tid];
        }
        if (k % probe == 0 || k == cg_max) {                                             // convergence probe: |r| <= 1e-13 |b|
            rb_dot(r, r, n, rnorm);
            int fin = 1;
            for (int c = 0; c < 3; ++c) if (act[c] && !(TRACK && cg_bad[c]) && cg_unfinished(rnorm[c], bnorm[c])) fin = 0;
            done = uni(fin);
            if (done || k == cg_max) break;
        }
    }
    __syncthreads();                                                                    // the last roll of rz is behind every thread
    cg.total += min(k, cg_max);                                                         // the true count rounded up to the probe interval
    for (int c = 0; c < 3; ++c) {
        const int bd = TRACK && cg_bad[c];
        bad_out[c] = act[c] && bd;
        if (act[c] && !bd && bnorm[c] > 0) { const double ratio = rnorm[c] / bnorm[c]; if (cg.worst_sq < ratio) cg.worst_sq = ratio; }
    }
    if (!done) ++cg.unconverged;
    __syncthreads();                                                                    // cgs and cg_bad are free again
}

// One Weighted-LAA step on the state s with the weights s.w; returns the score (the same in every thread; the caller looks at
// isfinite).  Expects a barrier behind the last write of Q and w; ends with one.
__device__ __forceinline__ double wg_laa_step(const WgLaa& s, int cg_max, WgCg& cg) {
    __shared__ double sh4[4];
    const int tid = threadIdx.x, l16 = tid & 15, row = tid >> 4;
    const int n = s.n, m = s.m;
    const int32_t *rowptr = s.rowptr, *eid = s.eid, *ii = s.ii, *jj = s.jj;
    const int8_t* sgn = s.sgn;
    Quat *QQ = s.QQ, *Q = s.Q;
    double *B = s.B, *w = s.w, *x = s.x, *rhs = s.rhs, *diag = s.diag, *Wv = s.Wv;
    // ---- Weighted_LAA: the edge log map, the normal equations
    for (int e = tid; e < m; e += 256) edge_log(QQ[e], Q[ii[e]], Q[jj[e]], B + 3 * (int64_t)e);
    __syncthreads();
    for (int vb = 0; vb < n; vb += 16) {
        const int v = vb + row;
        const bool on = v < n;
        double s3[3], dg;
        rhs_row16(eid, sgn, w, B, on ? rowptr[v] : 0, on ? rowptr[v + 1] : 0, l16, s3, &dg);
        if (on && l16 == 0) { rhs[3 * v] = s3[0]; rhs[3 * v + 1] = s3[1]; rhs[3 * v + 2] = s3[2]; diag[v] = dg; }
    }
    __syncthreads();
    // ---- laa_pcg<false, false> with laa_step's probe interval
    const int all[3] = {1, 1, 1};
    int bad[3];
    wg_pcg<false, false>(n, rowptr, s.adj, eid, w, rhs, diag, x, s.r, s.z, s.p, s.q, all, RB_PROBE, cg_max, cg, bad);
    // ---- Weighted_LAA.m:40-50: exp map, Q <- Q * W, the score in chunks of 256 rows
    double tot = 0.0;
    for (int base = 0; base < n; base += 256) {
        const int v = base + tid;
        double sc = 0.0;
        if (v < n) {
            const double theta = node_update(x + 3 * v, Q + v, Wv + 3 * v);
            if (v > 0) sc += theta;
        }
        tot += score_chunk_sum(sc, sh4);
        __syncthreads();
    }
    return tot / (double)n;
}

// The order statistics of the 0-based ranks k0 and, with next_too, k0 + 1 of RS[0..m) as order keys (key_value gives the doubles): an
// exact radix select, shared by wg_quantile below and k_align_batch's median (align_batch.hip).  k0 and next_too are the same in every
// thread; without next_too *key_hi = *key_lo.  RS may have been written just before the call without a barrier in between: the first
// barrier below orders it.  Returns 0, or 1 where the selection found no candidate (the same in every thread; the keys are then not
// written).  Every barrier it holds is passed by all threads or none.
__device__ __forceinline__ int wg_select(const double* RS, int m, int64_t k0, bool next_too, unsigned long long* key_lo, unsigned long long* key_hi) {
    __shared__ unsigned hist[256];
    __shared__ unsigned cnt_le;
    __shared__ unsigned long long key_gt;
    const int tid = threadIdx.x;
    // the order statistic of rank k0: radix select over the order key, most significant digit first
    unsigned long long prefix = 0;
    unsigned rank = (unsigned)k0;
    for (int pass = 7; pass >= 0; --pass) {
        const int shift = 8 * pass;
        hist[tid] = 0;
        __syncthreads();
        for (int e = tid; e < m; e += 256) {
            const unsigned long long key = order_key(RS[e]);
            if (pass == 7 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        unsigned acc = 0; int d = -1;
        for (int bin = 0; bin < 256; ++bin) {
            const unsigned hcount = hist[bin];
            if (d < 0) { if (acc + hcount > rank) d = bin; else acc += hcount; }
        }
        d = uni(d);
        __syncthreads();                                                                // hist is free again
        if (d < 0) return 1;
        rank -= uni((int)acc);
        prefix |= (unsigned long long)d << shift;
    }
    if (!next_too) { *key_lo = prefix; *key_hi = prefix; return 0; }
    // rank k0 + 1: the same value if more than k0 + 1 keys are <= it, else the smallest key above it
    if (tid == 0) { cnt_le = 0; key_gt = ~0ull; }
    __syncthreads();
    unsigned c_le = 0; unsigned long long k_gt = ~0ull;
    for (int e = tid; e < m; e += 256) {
        const unsigned long long key = order_key(RS[e]);
        if (key <= prefix) ++c_le; else if (key < k_gt) k_gt = key;
    }
    atomicAdd(&cnt_le, c_le);
    atomicMin(&key_gt, k_gt);
    __syncthreads();
    const unsigned le = cnt_le;
    const unsigned long long next = key_gt;
    __syncthreads();                                                                    // cnt_le, key_gt are free again
    unsigned long long upper = prefix;
    if (!uni(le >= (unsigned)k0 + 2u)) {
        if (uni(next == ~0ull)) return 1;
        upper = next;
    }
    *key_lo = prefix; *key_hi = upper;
    return 0;
}

// quantile(RS[0..m), p) into *thresh.  lo / hi: the extrema of this thread's entries (e = tid, tid + 256, ...); RS may have been
// written just before the call without a barrier in between: the first barrier below orders it.  Returns 0, or 1 where the selection
// found no candidate (the same in every thread; *thresh is then not written).  Every barrier it holds is passed by all threads or none.
__device__ __forceinline__ int wg_quantile(const double* RS, int m, double p, double lo, double hi, double* thresh) {
    __shared__ double mm[8];
    const int tid = threadIdx.x;
    for (int off = 32; off >= 1; off >>= 1) { lo = fmin(lo, __shfl_xor(lo, off)); hi = fmax(hi, __shfl_xor(hi, off)); }
    if ((tid & 63) == 0) { mm[tid >> 6] = lo; mm[4 + (tid >> 6)] = hi; }
    __syncthreads();                                                                    // RS, the wave extrema
    lo = fmin(fmin(mm[0], mm[1]), fmin(mm[2], mm[3])); hi = fmax(fmax(mm[4], mm[5]), fmax(mm[6], mm[7]));
    int64_t k0 = 0; double fr = 0.0;
    const int where = uni(hazen_position((int64_t)m, p, &k0, &fr));
    if (where == HAZEN_MIN) { *thresh = lo; return 0; }
    if (where == HAZEN_MAX) { *thresh = hi; return 0; }
    if (uni(hazen_flat(lo, hi))) { *thresh = lo; return 0; }
    unsigned long long prefix = 0, upper = 0;
    if (wg_select(RS, m, k0, true, &prefix, &upper)) return 1;
    *thresh = hazen_interp(key_value(prefix), key_value(upper), fr);
    return 0;
}

}  // namespace desc

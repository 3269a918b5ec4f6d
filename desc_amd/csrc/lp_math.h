// The arithmetic of the PDHG LP solver (linprog_sij) that the single-problem loop (lp.hip) and the batched one (lp_batch.hip) share: one
// text, so a problem gets the same bits whichever of them solves it (as pgd_math.h, laa_math.h and cemp_math.h for their callers).
//   lp_reduced_cost    1 + (K'y)_l of one variable, its incidence list summed by 16 lanes in a fixed order
//   lp_col_pass        x+ = clip(x - tau o (1 + K'y), 0, 1), xbar = 2 x+ - x, the running sum of x
//   lp_row_pass        y+ = max(y + sigma o (K xbar - b), 0), z = y1 + y2, own = sum_t (y1 - y2), the running sum of y
//   lp_eval_row_pass / lp_eval_col_pass / lp_eval_final   the certificates viol, b'y, P = sum x, sum min(0, reduced cost): block partials
//                      in block order, then one workgroup over the partials
//   lp_scan_block      the exclusive scan of the incidence counts by one workgroup, tau0 = 1 / (2 nsample + 2 count)
//   k_lp_count / k_lp_fill / k_lp_sort   the transposed incidence (every list ascending)
//   lp_decide          what the loop does after a check, from the two records: the scalar rule, host and device
// A pass is the work of block `blk` of a grid of `nblk` blocks of 256 threads over the mp variables that start at variable v0 and at
// cycle c0 of the arrays: the single call passes its launch grid and 0, 0; the batched call a grid per problem and the problem's offsets.
// The grid-stride order, and with it every sum, depends on (mp, nsample, nblk) alone.
#pragma once
#include <cmath>

#include "device_utils.h"

namespace desc {

struct LpRec { double viol, bty, P, dbox; double pad[4]; };      // the certificates of one point: 64 bytes

// ---- the scalar rule
__host__ __device__ inline double lp_dual_obj(const LpRec& r) { return -r.bty + r.dbox; }
__host__ __device__ inline double lp_error_of(const LpRec& r) {
    const double Dv = lp_dual_obj(r), gap = fabs(r.P - Dv) / (1.0 + fabs(r.P) + fabs(Dv));
    return r.viol < gap ? gap : r.viol;
}
__host__ __device__ inline bool lp_passes(const LpRec& r, double tol) {
    const double Dv = lp_dual_obj(r);
    return r.viol <= tol && r.P - Dv <= tol * (1.0 + fabs(r.P) + fabs(Dv));
}

struct LpLoop { double e_restart = INFINITY, e_prev = INFINITY; int32_t restarts = 0; };      // what the restart rule remembers between checks
enum { LP_CONTINUE = 0, LP_CONVERGED = 1, LP_RESTART_AVG = 2, LP_RESTART_CUR = 3 };
// The check at step `it`, `cnt` steps after the last restart.  cur: the iterate's record; avg: the running average's (read with
// `restart` only).  *use_avg: the average is the better point -- the candidate, and after LP_CONVERGED or at it == max_iter the returned
// one.  A restart updates s; the caller copies (LP_RESTART_AVG) or clears (LP_RESTART_CUR) and sets its cnt to 0.
__host__ __device__ inline int lp_decide(LpLoop& s, const LpRec& cur, const LpRec& avg, bool restart, double tol, int64_t cnt, int it, int max_iter, bool* use_avg) {
    *use_avg = restart && lp_error_of(avg) <= lp_error_of(cur);
    const LpRec& cand = *use_avg ? avg : cur;
    const double e = lp_error_of(cand);
    if (tol > 0.0 && lp_passes(cand, tol)) return LP_CONVERGED;
    if (!restart || it == max_iter) return LP_CONTINUE;
    if (e <= 0.2 * s.e_restart || (e <= 0.8 * s.e_restart && e > s.e_prev) || (double)cnt >= 0.36 * (double)it) {
        s.e_restart = e; s.e_prev = INFINITY; ++s.restarts;
        return *use_avg ? LP_RESTART_AVG : LP_RESTART_CUR;
    }
    s.e_prev = e;
    return LP_CONTINUE;
}

// ---- the transposed incidence: per variable the cycles in which it is the edge ik or jk
__global__ __launch_bounds__(256) static void k_lp_count(const int32_t* va, const int32_t* vb, int32_t* cnt, int64_t mc) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < mc; c += (int64_t)gridDim.x * 256) { atomicAdd(&cnt[va[c]], 1); atomicAdd(&cnt[vb[c]], 1); }
}
// exclusive scan of cnt[0 .. mp) into ptr[0 .. mp) by one workgroup of 1024 (a contiguous chunk per thread), starting at `base`; ptr[mp]
// = base + the total with write_end; tau0 = 1 / (2 nsample + 2 cnt); cnt is zeroed
__device__ __forceinline__ void lp_scan_block(int32_t* cnt, int32_t* ptr, double* tau0, int64_t mp, int nsample, int64_t base, bool write_end) {
    __shared__ int64_t s_sum[1024];
    const int64_t chunk = (mp + 1023) / 1024, lo0 = chunk * threadIdx.x, lo = lo0 < mp ? lo0 : mp, hi = lo + chunk < mp ? lo + chunk : mp;
    int64_t s = 0;
    for (int64_t l = lo; l < hi; ++l) s += cnt[l];
    s_sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { int64_t acc = 0; for (int t = 0; t < 1024; ++t) { const int64_t v = s_sum[t]; s_sum[t] = acc; acc += v; } if (write_end) ptr[mp] = (int32_t)(base + acc); }
    __syncthreads();
    int64_t acc = base + s_sum[threadIdx.x];
    for (int64_t l = lo; l < hi; ++l) {
        const int c = cnt[l];
        ptr[l] = (int32_t)acc; acc += c;
        tau0[l] = 1.0 / (2.0 * (double)nsample + 2.0 * (double)c);
        cnt[l] = 0;
    }
}
__global__ __launch_bounds__(256) static void k_lp_fill(const int32_t* va, const int32_t* vb, const int32_t* ptr, int32_t* cur, int32_t* list, int64_t mc) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < mc; c += (int64_t)gridDim.x * 256) {
        const int a = va[c], b = vb[c];
        list[ptr[a] + atomicAdd(&cur[a], 1)] = (int32_t)c;
        list[ptr[b] + atomicAdd(&cur[b], 1)] = (int32_t)c;
    }
}
// every list ascending (the fill's order is arrival order): rank sort by one wave per list, the list in the LDS when it fits.  The ids of
// one list are distinct (a cycle holds an edge once).
constexpr int LP_SORT_LDS = 2048;
__global__ __launch_bounds__(64) static void k_lp_sort(const int32_t* ptr, const int32_t* in, int32_t* out, int64_t mp) {
    __shared__ int32_t s_v[LP_SORT_LDS];
    for (int64_t l = blockIdx.x; l < mp; l += gridDim.x) {
        const int p0 = ptr[l], len = ptr[l + 1] - p0;
        const bool lds = len <= LP_SORT_LDS;
        __syncthreads();
        if (lds) for (int t = threadIdx.x; t < len; t += 64) s_v[t] = in[p0 + t];
        __syncthreads();
        for (int t = threadIdx.x; t < len; t += 64) {
            const int v = lds ? s_v[t] : in[p0 + t];
            int rank = 0;
            if (lds) for (int u = 0; u < len; ++u) rank += s_v[u] < v;
            else for (int u = 0; u < len; ++u) rank += in[p0 + u] < v;
            out[p0 + rank] = v;
        }
    }
}

// ---- the step
// reduced cost of variable l from z and own: 1 + (K'y)_l, the incidence list summed by the 16 lanes in a fixed order.  A group without
// a variable (!on) stays in the sum -- the DPP moves need every lane -- with an empty list: it loads nothing.
__device__ __forceinline__ double lp_reduced_cost(const int32_t* ptr, const int32_t* list, const double* z, const double* own, int64_t l, int sub, bool on) {
    const int p0 = on ? ptr[l] : 0, p1 = on ? ptr[l + 1] : 0;
    double acc = 0.0;
    for (int p = p0 + sub; p < p1; p += 16) acc += z[list[p]];
    acc = group_sum<16>(acc);
    return 1.0 + (on ? own[l] : 0.0) - acc;
}

template <bool AVG>
__device__ __forceinline__ void lp_col_pass(const int32_t* ptr, const int32_t* list, const double* z, const double* own, const double* tau0, double* x, double* xbar,
                                            double* xsum, int64_t mp, int blk, int nblk, int64_t v0) {
    const int sub = threadIdx.x & 15;
    const int64_t gid = ((int64_t)blk * 256 + threadIdx.x) >> 4, ng = ((int64_t)nblk * 256) >> 4;
    for (int64_t l0 = 0; l0 < mp; l0 += ng) {                   // whole waves stay in the loop: the DPP sums need every lane
        const bool on = l0 + gid < mp;
        const int64_t l = v0 + l0 + gid;
        const double rc = lp_reduced_cost(ptr, list, z, own, l, sub, on);
        if (on && sub == 0) {
            const double xo = x[l];
            const double xn = fmin(fmax(xo - tau0[l] * rc, 0.0), 1.0);
            x[l] = xn; xbar[l] = 2.0 * xn - xo;
            if (AVG) xsum[l] += xn;
        }
    }
}

// G lanes per variable, a cycle per lane; va / vb index xbar directly
template <int G, bool AVG>
__device__ __forceinline__ void lp_row_pass(const int32_t* va, const int32_t* vb, const double* S0, const double* xbar, double2* y, double2* ysum, double* z, double* own,
                                            double sigma, int64_t mp, int nsample, int blk, int nblk, int64_t v0, int64_t c0) {
    const int sub = threadIdx.x & (G - 1);
    const int64_t gid = ((int64_t)blk * 256 + threadIdx.x) / G, ng = ((int64_t)nblk * 256) / G;
    for (int64_t l0 = 0; l0 < mp; l0 += ng) {
        const int64_t l = l0 + gid;
        const bool on = l < mp;
        const double xl = on ? xbar[v0 + l] : 0.0;
        double acc = 0.0;
        if (on) for (int t = sub; t < nsample; t += G) {
            const int64_t c = c0 + l * nsample + t;
            const double s = xbar[va[c]] + xbar[vb[c]], d = S0[c];
            const double2 yo = y[c];
            double2 yn;
            yn.x = fmax(yo.x + sigma * ((xl - s) - d), 0.0);       // row  s_l - s_a - s_b <= d
            yn.y = fmax(yo.y + sigma * ((-xl - s) + d), 0.0);      // row -s_l - s_a - s_b <= -d
            y[c] = yn;
            z[c] = yn.x + yn.y;
            if (AVG) { double2 ys = ysum[c]; ys.x += yn.x; ys.y += yn.y; ysum[c] = ys; }
            acc += yn.x - yn.y;
        }
        acc = group_sum<G>(acc);
        if (on && sub == 0) own[v0 + l] = acc;
    }
}

// ---- the certificates of (x, y)
// first half: z and own of y, the block's partials of max violation and b'y into part[0], part[1]
template <int G>
__device__ __forceinline__ void lp_eval_row_pass(const int32_t* va, const int32_t* vb, const double* S0, const double* x, const double2* y, double* z, double* own,
                                                 double* part, int64_t mp, int nsample, int blk, int nblk, int64_t v0, int64_t c0) {
    const int sub = threadIdx.x & (G - 1);
    const int64_t gid = ((int64_t)blk * 256 + threadIdx.x) / G, ng = ((int64_t)nblk * 256) / G;
    double viol[1] = {0.0}, bty[1] = {0.0};
    for (int64_t l0 = 0; l0 < mp; l0 += ng) {
        const int64_t l = l0 + gid;
        const bool on = l < mp;
        const double xl = on ? x[v0 + l] : 0.0;
        double acc = 0.0;
        if (on) for (int t = sub; t < nsample; t += G) {
            const int64_t c = c0 + l * nsample + t;
            const double s = x[va[c]] + x[vb[c]], d = S0[c];
            const double2 yc = y[c];
            viol[0] = fmax(viol[0], fmax((xl - s) - d, (-xl - s) + d));
            bty[0] += d * (yc.x - yc.y);
            z[c] = yc.x + yc.y;
            acc += yc.x - yc.y;
        }
        acc = group_sum<G>(acc);
        if (on && sub == 0) own[v0 + l] = acc;
    }
    block_reduce<1, 2>(viol, part);
    __syncthreads();
    block_reduce<1, 0>(bty, part + 1);
}
// second half: the block's partials of sum x and sum min(0, reduced cost) into part[0], part[1]
__device__ __forceinline__ void lp_eval_col_pass(const int32_t* ptr, const int32_t* list, const double* z, const double* own, const double* x, double* part, int64_t mp,
                                                 int blk, int nblk, int64_t v0) {
    const int sub = threadIdx.x & 15;
    const int64_t gid = ((int64_t)blk * 256 + threadIdx.x) >> 4, ng = ((int64_t)nblk * 256) >> 4;
    double v[2] = {0.0, 0.0};
    for (int64_t l0 = 0; l0 < mp; l0 += ng) {
        const bool on = l0 + gid < mp;
        const int64_t l = v0 + l0 + gid;
        const double rc = lp_reduced_cost(ptr, list, z, own, l, sub, on);
        if (on && sub == 0) { v[0] += x[l]; v[1] += fmin(rc, 0.0); }
    }
    block_reduce<2, 0>(v, part);
}
// the partials of both halves in block order -> the record, by one workgroup of 256
__device__ __forceinline__ void lp_eval_final(const double* part_row, int nb_row, const double* part_col, int nb_col, LpRec* rec) {
    double a[1] = {0.0}, b[3] = {0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < nb_row; t += 256) { a[0] = fmax(a[0], part_row[2 * t]); b[0] += part_row[2 * t + 1]; }
    for (int t = threadIdx.x; t < nb_col; t += 256) { b[1] += part_col[2 * t]; b[2] += part_col[2 * t + 1]; }
    __shared__ double o[4];
    block_reduce<1, 2>(a, o);
    __syncthreads();
    block_reduce<3, 0>(b, o + 1);
    __syncthreads();
    if (threadIdx.x == 0) { rec->viol = o[0]; rec->bty = o[1]; rec->P = o[2]; rec->dbox = o[3]; }
}

// the running average since the last restart, and S_vec of a variable: clipped to the box
__device__ __forceinline__ double lp_average(double sum, double cnt) { return sum / cnt; }
__device__ __forceinline__ double lp_clip(double x) { return fmin(fmax(x, 0.0), 1.0); }

}  // namespace desc

// linprog_sij (Algorithms/linprog_sij.m:16-139): the LP relaxation of the corruption-estimation problem DESC solves as a QP,
//     min sum_l s_l   s.t.  |s_l - d_lt| <= s_a + s_b  for every sampled 3-cycle (l, t),   0 <= s <= 1,
// solved on the device by a matrix-free primal-dual hybrid gradient method (PDHG, the PDLP family) in f64.
//   :16-43    edges with cycles ("pos" edges, ascending edge order: the variables), nsample = max(ceil(median(codeg)/4), 30) -- the rule of
//             DESC_PGD.m:43, from the codegree histogram of the sampler (no PGD structure is built)
//   :64-102   nsample cycles per pos edge WITH replacement and S0Mat: cemp_build (cemp.hip, CEMP.m:62-101 is the same text); the t-th sample of
//             edge l is CoInd[desc_sample_key(seed, l, t) mod codeg].  Duplicate samples are duplicate rows: they do not change the LP.
//   :104      edges without a cycle keep S_vec = 1; they are no variables, and no row references them (ik and jk lie on the triangle)
//   :107-136  per cycle c = (l, t) with d = S0Mat(t, l), a = edge {i,k}, b = edge {j,k}, two rows: s_l - s_a - s_b <= d and -s_l - s_a - s_b <= -d
// One deliberate departure: :84-85 index Ind_i(l) / Ind_j(l) with l running over the pos edges, which is the wrong edge as soon as some edge
// has no cycle.  The edge's own endpoints are used (as :66 and CEMP.m do); the two agree whenever every edge lies on a triangle.
//
// The solver.  K never exists: a row is a cycle, its three columns are CempState's index arrays.  With c = 1 the recurrence is
//     x+ = clip(x - tau o (1 + K'y), 0, 1),      y+ = max(y + sigma o (K (2 x+ - x) - b), 0)
// with the diagonal steps of Pock & Chambolle (alpha = 1):  tau_l = 1 / sum_r |K_rl| = 1 / (2 nsample + 2 inc_l), inc_l = the cycles in which
// l is ik or jk;  sigma_r = 1 / sum_l |K_rl| = 1 / 3.
//   k_lp_col   per pos edge (16 lanes): gathers z_c = y1 + y2 over the edge's incidence list -- a CSR built once per call, cycle ids ascending,
//              so the order of the sum is fixed and K'y needs no floating-point atomics --, reduced cost 1 + own - sum z, clipped step, writes x,
//              xbar = 2 x+ - x and the running sum of x
//   k_lp_row   per pos edge (32 or 64 lanes, a cycle per lane): gathers xbar[a], xbar[b], updates both duals, writes z_c, the running sum of y
//              and own_l = sum_t (y1 - y2)
// Every check_every steps the certificates of the iterate and of the running average since the last restart are evaluated on the device
// (k_lp_eval_row / k_lp_eval_col, fixed-order block partials, one 64-byte record read by the host):
//     viol = max_r max((Kx - b)_r, 0),   P = sum x,   D = -b'y + sum_l min(0, 1 + (K'y)_l)      (every y >= 0 is dual feasible: D <= f*)
// and the run stops when viol <= tol and P - D <= tol (1 + |P| + |D|) for one of the two (that one is returned).  Restarts follow PDLP
// (Applegate et al. 2021) with the error e = max(viol, |P - D| / (1 + |P| + |D|)): the better of iterate and average becomes the new start
// when e <= 0.2 e_restart, or e <= 0.8 e_restart and e grew since the last check, or the period is >= 0.36 of all steps.  PDLP's primal
// weight is left out: updated from the moves between restarts it made a NumPy model of this loop 2 to 8 times slower on the test graphs
// (the gap then lags the violation).  Defaults: tol 1e-4, max_iter 200000, check_every 64.  restart = 0 keeps no averages; with tol = 0
// besides, exactly max_iter plain steps run from x = 0, y = 0.
// Two runs on the same input return the same bits: no atomics on doubles, fixed reduction trees, grids that depend on the sizes only.
// The kernels' arithmetic and the rule the host applies after a check (lp_decide) are lp_math.h's: lp_batch.hip runs the same text for many
// small problems at once, and a problem gets the same bits from either.
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "cemp_state.h"
#include "lp_math.h"

namespace desc {
namespace {

// variable (pos index) of the two other edges of every cycle
__global__ __launch_bounds__(256) void k_lp_vars(const int32_t* e_ki, const int32_t* e_jk, const int32_t* poe, int32_t* va, int32_t* vb, int64_t mc) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < mc; c += (int64_t)gridDim.x * 256) { va[c] = poe[e_ki[c]]; vb[c] = poe[e_jk[c]]; }
}
__global__ __launch_bounds__(1024) void k_lp_scan(int32_t* cnt, int32_t* ptr, double* tau0, int64_t mp, int nsample) { lp_scan_block(cnt, ptr, tau0, mp, nsample, 0, true); }

// the kernels of the loop: the passes of lp_math.h over the launch grid, the problem at variable 0 and cycle 0 of its arrays
template <bool AVG>
__global__ __launch_bounds__(256) void k_lp_col(const int32_t* ptr, const int32_t* list, const double* z, const double* own, const double* tau0,
                                                double* x, double* xbar, double* xsum, int64_t mp) {
    lp_col_pass<AVG>(ptr, list, z, own, tau0, x, xbar, xsum, mp, blockIdx.x, gridDim.x, 0);
}
template <int G, bool AVG>
__global__ __launch_bounds__(256) void k_lp_row(const int32_t* va, const int32_t* vb, const double* S0, const double* xbar, double2* y, double2* ysum, double* z,
                                                double* own, double sigma, int64_t mp, int nsample) {
    lp_row_pass<G, AVG>(va, vb, S0, xbar, y, ysum, z, own, sigma, mp, nsample, blockIdx.x, gridDim.x, 0, 0);
}
template <int G>
__global__ __launch_bounds__(256) void k_lp_eval_row(const int32_t* va, const int32_t* vb, const double* S0, const double* x, const double2* y, double* z, double* own,
                                                     double* part, int64_t mp, int nsample) {
    lp_eval_row_pass<G>(va, vb, S0, x, y, z, own, part + 2 * blockIdx.x, mp, nsample, blockIdx.x, gridDim.x, 0, 0);
}
__global__ __launch_bounds__(256) void k_lp_eval_col(const int32_t* ptr, const int32_t* list, const double* z, const double* own, const double* x, double* part, int64_t mp) {
    lp_eval_col_pass(ptr, list, z, own, x, part + 2 * blockIdx.x, mp, blockIdx.x, gridDim.x, 0);
}
__global__ __launch_bounds__(256) void k_lp_eval_final(const double* part_row, int nb_row, const double* part_col, int nb_col, LpRec* rec) {
    lp_eval_final(part_row, nb_row, part_col, nb_col, rec);
}

__global__ __launch_bounds__(256) void k_lp_average(const double* sum, double* out, double cnt, int64_t count) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < count; t += (int64_t)gridDim.x * 256) out[t] = lp_average(sum[t], cnt);
}
// restart: v <- src, the running sum cleared
__global__ __launch_bounds__(256) void k_lp_restart(const double* src, double* v, double* sum, int64_t count) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < count; t += (int64_t)gridDim.x * 256) { v[t] = src[t]; sum[t] = 0.0; }
}
__global__ __launch_bounds__(256) void k_lp_set(double* p, int64_t count, double v) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < count; t += (int64_t)gridDim.x * 256) p[t] = v;
}
// S_vec: 1 without a cycle (:104), the variable clipped to the box otherwise
__global__ __launch_bounds__(256) void k_lp_out(const int32_t* pos, const double* x, double* s_vec, int64_t mp) {
    for (int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x; l < mp; l += (int64_t)gridDim.x * 256) s_vec[pos[l]] = lp_clip(x[l]);
}

struct LpTimer {                                        // hipEvent laps of the loop's two kernels (verbose >= 2: tools/lp_stages.py)
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    double ms_col = 0.0, ms_row = 0.0; int laps = 0;
    ~LpTimer() { for (auto q : e) if (q) (void)hipEventDestroy(q); }
};

}  // namespace
}  // namespace desc

using namespace desc;

extern "C" void desc_lp_params_default(desc_lp_params* p) {
    if (!p) return;
    p->nsample = 0; p->check_every = 64; p->seed = 0; p->tol = 1e-4; p->max_iter = 200000; p->restart = 1; p->verbose = 0; p->reserved = 0; p->pos_out = nullptr;
}

extern "C" int desc_lp_sij_run(const desc_problem* prob, const desc_lp_params* params, int32_t device, double* s_vec, double* y, int32_t* k_out,
                               desc_lp_info* info) {
    if (!prob || !s_vec) return fail(DESC_ERR_INVALID, "NULL argument");
    auto t0 = std::chrono::steady_clock::now();
    const int rc = with_uploaded(prob, device, [&](const desc_device_problem* dp) { return desc_lp_sij_run_dev(dp, params, s_vec, y, k_out, info); });
    if (!rc && info) info->ms_total = ms_since(t0);
    return rc;
}

extern "C" int desc_lp_sij_run_dev(const desc_device_problem* dp, const desc_lp_params* params, double* s_vec, double* y_out, int32_t* k_out,
                                   desc_lp_info* info) {
    return no_throw("desc_lp_sij_run_dev", [&]() -> int {
    if (!dp || !s_vec) return fail(DESC_ERR_INVALID, "NULL argument");
    desc_lp_params P;
    desc_lp_params_default(&P);
    if (params) P = *params;
    if (P.nsample < 0 || P.max_iter < 0 || P.check_every < 0 || !(P.tol >= 0.0)) return fail(DESC_ERR_INVALID, "need nsample >= 0, max_iter >= 0, check_every >= 0, tol >= 0");
    if (P.check_every == 0) P.check_every = 64;
    const int64_t m = dp->m;
    if (dp->n < 1 || m < 1) return fail(DESC_ERR_INVALID, "empty graph");
    int rc = DESC_OK;
    DESC_HIP(hipSetDevice(dp->device));
    auto t0 = std::chrono::steady_clock::now();
    // ---- samples and S0Mat (:16-102)
    CempState cs;
    if ((rc = cemp_build(dp, P.nsample, P.seed, true, cs))) return rc;
    DESC_HIP(hipDeviceSynchronize());
    const double ms_samples = ms_since(t0);
    const int64_t mp = cs.mp, mc = cs.mc;
    const int nsample = cs.nsample;
    if (2 * mc >= (1ll << 31)) return fail(DESC_ERR_TOO_LARGE, "2 * m_pos * nsample exceeds 2^31");
    desc_lp_info I{};
    I.nsample = nsample; I.m_pos = mp; I.rows = 2 * mc; I.ms_samples = ms_samples;
    DevArena D;
    double* d_svec;
    if ((rc = D.alloc(&d_svec, m))) return rc;
    hipLaunchKernelGGL(k_lp_set, dim3(grid_for(m, 1024)), dim3(256), 0, 0, d_svec, m, 1.0);           // :104
    if (mp == 0 || (P.max_iter == 0 && !y_out && !k_out && !P.pos_out)) {                                            // no variable: the empty LP; no step, no output: the sizes
        I.converged = mp == 0;
        DESC_HIP(hipMemcpy(s_vec, d_svec, sizeof(double) * m, hipMemcpyDeviceToHost));
        I.ms_total = ms_since(t0);
        if (info) *info = I;
        return DESC_OK;
    }
    // ---- the transposed incidence (built once per call)
    auto t1 = std::chrono::steady_clock::now();
    const int32_t *d_va = cs.d_eki, *d_vb = cs.d_ejk;                                                  // every edge a variable: the edge ids themselves
    const int cgrid = grid_for(mc, 4096);
    if (cs.d_poe) {
        int32_t *va, *vb;
        if ((rc = D.alloc(&va, mc)) || (rc = D.alloc(&vb, mc))) return rc;
        hipLaunchKernelGGL(k_lp_vars, dim3(cgrid), dim3(256), 0, 0, cs.d_eki, cs.d_ejk, cs.d_poe, va, vb, mc);
        d_va = va; d_vb = vb;
    }
    int32_t *d_cnt, *d_ptr, *d_list0, *d_list;
    double* d_tau0;
    if ((rc = D.alloc(&d_cnt, mp)) || (rc = D.alloc(&d_ptr, mp + 1)) || (rc = D.alloc(&d_list0, 2 * mc)) || (rc = D.alloc(&d_list, 2 * mc)) || (rc = D.alloc(&d_tau0, mp))) return rc;
    DESC_HIP(hipMemsetAsync(d_cnt, 0, sizeof(int32_t) * mp, 0));
    hipLaunchKernelGGL(k_lp_count, dim3(cgrid), dim3(256), 0, 0, d_va, d_vb, d_cnt, mc);
    hipLaunchKernelGGL(k_lp_scan, dim3(1), dim3(1024), 0, 0, d_cnt, d_ptr, d_tau0, mp, nsample);
    hipLaunchKernelGGL(k_lp_fill, dim3(cgrid), dim3(256), 0, 0, d_va, d_vb, d_ptr, d_cnt, d_list0, mc);
    hipLaunchKernelGGL(k_lp_sort, dim3((unsigned)std::min<int64_t>(mp, 65536)), dim3(64), 0, 0, d_ptr, d_list0, d_list, mp);
    DESC_HIP(hipGetLastError());
    DESC_HIP(hipDeviceSynchronize());
    I.ms_transpose = ms_since(t1);
    // ---- the loop
    auto t2 = std::chrono::steady_clock::now();
    const bool restart = P.restart != 0, checks = restart || P.tol > 0.0;
    double *d_x, *d_xbar, *d_own, *d_z, *d_y;
    double *d_xs = nullptr, *d_ys = nullptr, *d_xa = nullptr, *d_ya = nullptr, *d_zt, *d_ownt, *d_part_row, *d_part_col;
    LpRec* d_rec;
    const int ncol = grid_for(mp, 2048, 16), nrow64 = grid_for(mp, 4096, 4), nrow32 = grid_for(mp, 4096, 8);
    const bool g32 = nsample <= 32;
    const int nrow = g32 ? nrow32 : nrow64;
    if ((rc = D.alloc(&d_x, mp)) || (rc = D.alloc(&d_xbar, mp)) || (rc = D.alloc(&d_own, mp)) || (rc = D.alloc(&d_z, mc)) || (rc = D.alloc(&d_y, 2 * mc)) ||
        (rc = D.alloc(&d_zt, mc)) || (rc = D.alloc(&d_ownt, mp)) || (rc = D.alloc(&d_part_row, 2 * (size_t)nrow)) || (rc = D.alloc(&d_part_col, 2 * (size_t)ncol)) ||
        (rc = D.alloc(&d_rec, 1))) return rc;
    if (restart && ((rc = D.alloc(&d_xs, mp)) || (rc = D.alloc(&d_ys, 2 * mc)) || (rc = D.alloc(&d_xa, mp)) || (rc = D.alloc(&d_ya, 2 * mc)))) return rc;
    for (double* q : {d_x, d_xbar, d_own, d_xs}) if (q) DESC_HIP(hipMemsetAsync(q, 0, sizeof(double) * mp, 0));
    DESC_HIP(hipMemsetAsync(d_z, 0, sizeof(double) * mc, 0));
    for (double* q : {d_y, d_ys}) if (q) DESC_HIP(hipMemsetAsync(q, 0, sizeof(double) * 2 * mc, 0));
    LpTimer tm;
    const bool laps = P.verbose >= 2;
    if (laps) for (auto& q : tm.e) DESC_HIP(hipEventCreate(&q));
    auto evaluate = [&](const double* x, const double* y, LpRec* out) -> int {                         // z / own of y land in d_zt / d_ownt
        if (g32) hipLaunchKernelGGL((k_lp_eval_row<32>), dim3(nrow), dim3(256), 0, 0, d_va, d_vb, cs.d_S0, x, (const double2*)y, d_zt, d_ownt, d_part_row, mp, nsample);
        else hipLaunchKernelGGL((k_lp_eval_row<64>), dim3(nrow), dim3(256), 0, 0, d_va, d_vb, cs.d_S0, x, (const double2*)y, d_zt, d_ownt, d_part_row, mp, nsample);
        hipLaunchKernelGGL(k_lp_eval_col, dim3(ncol), dim3(256), 0, 0, d_ptr, d_list, d_zt, d_ownt, x, d_part_col, mp);
        hipLaunchKernelGGL(k_lp_eval_final, dim3(1), dim3(256), 0, 0, d_part_row, nrow, d_part_col, ncol, d_rec);
        DESC_HIP(hipMemcpy(out, d_rec, sizeof(LpRec), hipMemcpyDeviceToHost));
        return DESC_OK;
    };
    LpLoop loop;                                           // the restart rule's memory (lp_math.h: lp_decide)
    int64_t cnt = 0;
    int it = 0;
    bool converged = false;
    const double *x_fin = d_x, *y_fin = d_y;
    LpRec fin{};
    bool have_fin = false;
    while (it < P.max_iter) {
        ++it;
        if (laps) DESC_HIP(hipEventRecord(tm.e[0], 0));
        if (restart) hipLaunchKernelGGL(k_lp_col<true>, dim3(ncol), dim3(256), 0, 0, d_ptr, d_list, d_z, d_own, d_tau0, d_x, d_xbar, d_xs, mp);
        else hipLaunchKernelGGL(k_lp_col<false>, dim3(ncol), dim3(256), 0, 0, d_ptr, d_list, d_z, d_own, d_tau0, d_x, d_xbar, d_xs, mp);
        if (laps) DESC_HIP(hipEventRecord(tm.e[1], 0));
        const double sigma = 1.0 / 3.0;
        if (g32) {
            if (restart) hipLaunchKernelGGL((k_lp_row<32, true>), dim3(nrow), dim3(256), 0, 0, d_va, d_vb, cs.d_S0, d_xbar, (double2*)d_y, (double2*)d_ys, d_z, d_own, sigma, mp, nsample);
            else hipLaunchKernelGGL((k_lp_row<32, false>), dim3(nrow), dim3(256), 0, 0, d_va, d_vb, cs.d_S0, d_xbar, (double2*)d_y, (double2*)d_ys, d_z, d_own, sigma, mp, nsample);
        } else {
            if (restart) hipLaunchKernelGGL((k_lp_row<64, true>), dim3(nrow), dim3(256), 0, 0, d_va, d_vb, cs.d_S0, d_xbar, (double2*)d_y, (double2*)d_ys, d_z, d_own, sigma, mp, nsample);
            else hipLaunchKernelGGL((k_lp_row<64, false>), dim3(nrow), dim3(256), 0, 0, d_va, d_vb, cs.d_S0, d_xbar, (double2*)d_y, (double2*)d_ys, d_z, d_own, sigma, mp, nsample);
        }
        if (laps) {
            DESC_HIP(hipEventRecord(tm.e[2], 0));
            DESC_HIP(hipEventSynchronize(tm.e[2]));
            float a = 0.f, b = 0.f;
            DESC_HIP(hipEventElapsedTime(&a, tm.e[0], tm.e[1])); DESC_HIP(hipEventElapsedTime(&b, tm.e[1], tm.e[2]));
            tm.ms_col += a; tm.ms_row += b; ++tm.laps;
        }
        ++cnt;
        if (!checks || (it % P.check_every != 0 && it != P.max_iter)) continue;
        LpRec rc_cur, rc_avg{};
        if ((rc = evaluate(d_x, d_y, &rc_cur))) return rc;
        bool use_avg = false;
        if (restart) {
            hipLaunchKernelGGL(k_lp_average, dim3(grid_for(mp, 1024)), dim3(256), 0, 0, d_xs, d_xa, (double)cnt, mp);
            hipLaunchKernelGGL(k_lp_average, dim3(grid_for(2 * mc, 1024)), dim3(256), 0, 0, d_ys, d_ya, (double)cnt, 2 * mc);
            if ((rc = evaluate(d_xa, d_ya, &rc_avg))) return rc;                                       // last: d_zt / d_ownt belong to the average
        }
        const int act = lp_decide(loop, rc_cur, rc_avg, restart, P.tol, cnt, it, P.max_iter, &use_avg);
        const LpRec& cand = use_avg ? rc_avg : rc_cur;
        if (P.verbose) printf("lp iter %d: viol %.3e  P %.9g  D %.9g  err %.3e  %s  restarts %d\n", it, cand.viol, cand.P, lp_dual_obj(cand), lp_error_of(cand), use_avg ? "avg" : "cur",
                              loop.restarts - (act == LP_RESTART_AVG || act == LP_RESTART_CUR ? 1 : 0));
        fin = cand; have_fin = true; x_fin = use_avg ? d_xa : d_x; y_fin = use_avg ? d_ya : d_y;
        if (act == LP_CONVERGED) { converged = true; break; }
        if (act == LP_CONTINUE) continue;
        if (act == LP_RESTART_AVG) {
            hipLaunchKernelGGL(k_lp_restart, dim3(grid_for(mp, 1024)), dim3(256), 0, 0, d_xa, d_x, d_xs, mp);
            hipLaunchKernelGGL(k_lp_restart, dim3(grid_for(2 * mc, 1024)), dim3(256), 0, 0, d_ya, d_y, d_ys, 2 * mc);
            std::swap(d_z, d_zt); std::swap(d_own, d_ownt);                                          // z / own of the new y
        } else {
            DESC_HIP(hipMemsetAsync(d_xs, 0, sizeof(double) * mp, 0));
            DESC_HIP(hipMemsetAsync(d_ys, 0, sizeof(double) * 2 * mc, 0));
        }
        x_fin = d_x; y_fin = d_y;
        cnt = 0;
    }
    if (!have_fin) { if ((rc = evaluate(d_x, d_y, &fin))) return rc; x_fin = d_x; y_fin = d_y; }
    hipLaunchKernelGGL(k_lp_out, dim3(grid_for(mp, 1024)), dim3(256), 0, 0, cs.d_pos, x_fin, d_svec, mp);
    DESC_HIP(hipGetLastError());
    DESC_HIP(hipDeviceSynchronize());
    DESC_HIP(hipMemcpy(s_vec, d_svec, sizeof(double) * m, hipMemcpyDeviceToHost));
    if (y_out) DESC_HIP(hipMemcpy(y_out, y_fin, sizeof(double) * 2 * mc, hipMemcpyDeviceToHost));
    if (P.pos_out) DESC_HIP(hipMemcpy(P.pos_out, cs.d_pos, sizeof(int32_t) * mp, hipMemcpyDeviceToHost));
    if (k_out) {
        DESC_HIP(hipMemcpy(k_out, cs.d_k, sizeof(int32_t) * mc, hipMemcpyDeviceToHost));
        for (int64_t c = 0; c < mc; ++c) k_out[c] += 1;                                                // 1-based, as CoIndMat
    }
    I.iters = it; I.restarts = loop.restarts; I.converged = converged ? 1 : 0;
    I.viol = fin.viol; I.pobj = fin.P; I.dobj = lp_dual_obj(fin);
    I.ms_loop = ms_since(t2); I.ms_total = ms_since(t0);
    if (tm.laps) { I.ms_col = tm.ms_col / tm.laps; I.ms_row = tm.ms_row / tm.laps; }
    if (!converged && P.tol > 0.0)
        fprintf(stderr, "[desc_amd] linprog_sij: the LP solver stopped at max_iter = %d with viol %.3e, P %.9g, D %.9g (tol %.1e): S_vec is the better of the last iterate and the running average\n",
                P.max_iter, fin.viol, fin.P, lp_dual_obj(fin), P.tol);
    if (P.verbose) fflush(stdout);
    if (info) *info = I;
    return DESC_OK;
    });
}

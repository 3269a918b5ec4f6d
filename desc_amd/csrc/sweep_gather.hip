// GATHER layout of the PGD sweep (see pgd.hip): its kernels, instance table and launcher, and the handle's setup on that layout.
#include <chrono>

#include "pgd_handle.h"

namespace desc {

// ===========================================================================
// GATHER variant
// ===========================================================================
template <int G, int STEP>
__global__ __launch_bounds__(256) void k_sweep(SweepArgs a) {
    if (a.state->stop) return;
    constexpr int EPW = 64 / G;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int sub = lane / G, gl = lane % G;
    const int nb = gridDim.x;
    const int lb = xcd_logical_block(blockIdx.x, nb);
    const int per_block = (a.m_pos + nb - 1) / nb;
    const int lo_edge = lb * per_block;
    const int hi_edge = min(a.m_pos, lo_edge + per_block);

    double obj_acc = 0.0, chg_acc = 0.0;
    for (int l0 = lo_edge + wv * EPW; l0 < hi_edge; l0 += 4 * EPW) {
        const int l = l0 + sub;
        const bool edge_ok = l < hi_edge;
        int base = 0, cnt = 0;
        if (edge_ok) { base = a.cum[l]; cnt = a.cum[l + 1] - base; }
        const bool act0 = gl < cnt;
        const int64_t c = (int64_t)base + gl;

        double w = 0.0, d = 0.0, ssum = 0.0, wa = 0.0, wb = 0.0;
        int ia = -1, ib = -1;
        if (act0) {
            const int ejk = a.e_jk[c], eki = a.e_ki[c];
            ia = a.ikj[c]; ib = a.jki[c];
            w = a.w_old[c]; d = a.S0[c];
            ssum = a.S_old[ejk] + a.S_old[eki];
            if (ia >= 0) wa = a.w_old[ia];
            if (ib >= 0) wb = a.w_old[ib];
        }
        obj_acc += w * ssum;                       // objective of the iterate being read (:233, one sweep late)
        // mirror-weight sums: one scalar per edge, applied to masked positions only (:189-190)
        const double T1 = group_sum<G>(wa), T2 = group_sum<G>(wb);
        double g = ssum + ((ia >= 0 ? T1 : 0.0) + (ib >= 0 ? T2 : 0.0)) * d;          // :193
        // tangent projection grad - (grad*nv')*nv, nv = ones/sqrt(cnt)  (:199-201)
        const double nv = act0 ? a.nv_tab[cnt] : 0.0;
        const double dot = group_sum<G>(act0 ? g * nv : 0.0);
        g = g - dot * nv;
        const double ws = act0 ? apply_step<STEP>(a.st, w, g, c) : 0.0;               // :207
        const double T = simplex_threshold<G>(ws, act0, lane);          // :215-223
        const double wn = act0 ? fmax(ws - T, 0.0) : 0.0;                             // :224
        const double snew = group_sum<G>(wn * d);                                     // :229
        if (act0) a.w_new[c] = wn;
        if (edge_ok && gl == 0) {
            const int e = a.pos_edge[l];
            chg_acc += fabs(snew - a.S_old[e]);                                       // :232
            a.S_new[e] = snew;
        }
    }
    block_partials(obj_acc, chg_acc, a.partials, lb);
}

// Segments longer than 64 cycles: one wave per edge, several passes over the segment;
// w_new doubles as scratch (each lane re-reads only what it wrote itself).
template <int STEP>
__global__ __launch_bounds__(256) void k_sweep_big(SweepArgs a) {
    if (a.state->stop) return;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int nb = gridDim.x;
    const int lb = xcd_logical_block(blockIdx.x, nb);
    const int per_block = (a.m_pos + nb - 1) / nb;
    const int lo_edge = lb * per_block;
    const int hi_edge = min(a.m_pos, lo_edge + per_block);

    double obj_acc = 0.0, chg_acc = 0.0;
    for (int l = lo_edge + wv; l < hi_edge; l += 4) {
        const int base = a.cum[l], cnt = a.cum[l + 1] - base;
        double t1 = 0.0, t2 = 0.0;
        for (int t = lane; t < cnt; t += 64) {
            const int64_t c = (int64_t)base + t;
            const int ia = a.ikj[c], ib = a.jki[c];
            if (ia >= 0) t1 += a.w_old[ia];
            if (ib >= 0) t2 += a.w_old[ib];
        }
        const double T1 = group_sum<64>(t1), T2 = group_sum<64>(t2);
        const double nv = a.nv_tab[cnt];
        double dotp = 0.0;
        for (int t = lane; t < cnt; t += 64) {
            const int64_t c = (int64_t)base + t;
            const double ssum = a.S_old[a.e_jk[c]] + a.S_old[a.e_ki[c]];
            obj_acc += a.w_old[c] * ssum;
            const double g = ssum + ((a.ikj[c] >= 0 ? T1 : 0.0) + (a.jki[c] >= 0 ? T2 : 0.0)) * a.S0[c];
            a.w_new[c] = g;
            dotp += g * nv;
        }
        const double dot = group_sum<64>(dotp);
        for (int t = lane; t < cnt; t += 64) {
            const int64_t c = (int64_t)base + t;
            const double g = a.w_new[c] - dot * nv;
            a.w_new[c] = apply_step<STEP>(a.st, a.w_old[c], g, c);
        }
        double T = -INFINITY;
        int prev_n = -1;
        for (;;) {
            double s = 0.0; int na = 0;
            for (int t = lane; t < cnt; t += 64) {
                const double x = a.w_new[(int64_t)base + t];
                if (x > T) { s += x; ++na; }
            }
            s = group_sum<64>(s);
            na = (int)group_sum<64>((double)na);
            if (na == prev_n) break;
            prev_n = na;
            T = (s - 1.0) / (double)max(na, 1);
        }
        double sn = 0.0;
        for (int t = lane; t < cnt; t += 64) {
            const int64_t c = (int64_t)base + t;
            const double wn = fmax(a.w_new[c] - T, 0.0);
            a.w_new[c] = wn;
            sn += wn * a.S0[c];
        }
        const double snew = group_sum<64>(sn);
        if (lane == 0) {
            const int e = a.pos_edge[l];
            chg_acc += fabs(snew - a.S_old[e]);
            a.S_new[e] = snew;
        }
    }
    block_partials(obj_acc, chg_acc, a.partials, lb);
}

// Cycle inconsistency (DESC_PGD.m:129-147): one wave per edge, lanes over its cycles.
// R_jk = RijMat4d(:,:,j,k) is the stored block of edge {j,k} if j<k, its transpose
// otherwise; likewise R_ki (:65-66,89-91).
__global__ __launch_bounds__(256) void k_cycle_d(const int32_t* cum, const int32_t* pos_edge, const int32_t* ind_i,
                                                 const int32_t* ind_j, const int32_t* kk, const int32_t* e_jk,
                                                 const int32_t* e_ki, const double* rij, double* S0, int m_pos) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t l = wid; l < m_pos; l += nw) {
        const int base = cum[l], cnt = cum[l + 1] - base;
        const int e = pos_edge[l], i = ind_i[e], j = ind_j[e];
        double A[9];
        for (int t = 0; t < 9; ++t) A[t] = rij[9 * (int64_t)e + t];
        for (int q = lane; q < cnt; q += 64) {
            const int64_t c = (int64_t)base + q;
            const int k = kk[c];
            const double tr = cycle_trace(A, rij + 9 * (int64_t)e_jk[c], !(j < k), rij + 9 * (int64_t)e_ki[c], !(k < i));
            S0[c] = abs_acos_ext((tr - 1.0) / 2.0) / M_PI;
        }
    }
}

namespace {

// gather layout: G lanes per segment; above 64 cycles (G = 0) k_sweep_big, the multi-pass wave-per-edge kernel
template <int G>
constexpr SweepInst<SweepArgs> gather_inst() { return {{G, 0}, 256, {k_sweep<G, DESC_STEP_CONSTANT>, k_sweep<G, DESC_STEP_HYBRID>}}; }
constexpr SweepInst<SweepArgs> big_inst() { return {{0, 0}, 256, {k_sweep_big<DESC_STEP_CONSTANT>, k_sweep_big<DESC_STEP_HYBRID>}}; }
const SweepInst<SweepArgs> GATHER_INSTS[] = {gather_inst<16>(), gather_inst<32>(), gather_inst<64>(), big_inst()};
SweepShape gather_shape(int c) { return {c <= 16 ? 16 : c <= 32 ? 32 : c <= 64 ? 64 : 0, 0}; }      // 16, 32, 64 or 0: each has its entry
std::string gather_prefix(SweepShape sh) { return sh.lps ? inst_name("k_sweep<%d,", sh.lps) : std::string("k_sweep_big<"); }

int choose_grid(desc_pgd* h) {
    const int G = gather_shape(h->max_cnt).lps, epw = G ? 64 / G : 1;
    int64_t want = (h->m_pos + 4 * epw - 1) / (4 * epw);
    want = std::min<int64_t>(want, 2048);
    want = std::max<int64_t>(want, 8);
    h->grid = (int)((want + 7) / 8 * 8);
    return DESC_OK;
}

}  // namespace

int launch_gather(desc_pgd* h, const SweepArgs& a, bool adam) {
    const auto* k = sweep_inst(GATHER_INSTS, gather_shape(h->max_cnt));
    if (!k) return DESC_ERR_STATE;
    h->last_sweep = gather_prefix(k->sh) + inst_name("%d>", STEP_OF[adam]);
    hipLaunchKernelGGL(k->kern[adam], dim3(h->grid), dim3(k->NT), 0, h->stream, a);
    return DESC_OK;
}

// ---------------------------------------------------------------- GATHER setup
int setup_gather(desc_pgd* h, const desc_problem* prob, const desc_structure* s, const double* shared_rij) {
    const int64_t m = h->m, mp = h->m_pos, mc = h->m_cycle;
    int rc;
    if ((rc = structure_ensure_host(const_cast<desc_structure*>(s)))) return rc;
    if ((rc = dalloc(h, &h->d_pos_edge, mp))) return rc;
    if ((rc = dalloc(h, &h->d_ejk, mc))) return rc;
    if ((rc = dalloc(h, &h->d_eki, mc))) return rc;
    if ((rc = dalloc(h, &h->d_ikj, mc))) return rc;
    if ((rc = dalloc(h, &h->d_jki, mc))) return rc;
    if ((rc = dalloc(h, &h->d_S[0], m))) return rc;
    if ((rc = dalloc(h, &h->d_S[1], m))) return rc;
    choose_grid(h);
    h->obj_grid = (int)std::min<int64_t>(2048, std::max<int64_t>(1, (mc + 255) / 256));
    h->kname = gather_prefix(gather_shape(h->max_cnt));

    auto t0 = std::chrono::steady_clock::now();
    hvec<int32_t> cum32((size_t)mp + 1);
    for (int64_t l = 0; l <= mp; ++l) cum32[l] = (int32_t)s->cum_ind[l];
    int32_t *d_k = nullptr, *d_ii = nullptr, *d_jj = nullptr; double* d_rij = nullptr;
    if ((rc = dalloc(h, &d_k, mc))) return rc;
    if ((rc = dalloc(h, &d_ii, m))) return rc;
    if ((rc = dalloc(h, &d_jj, m))) return rc;
    if (shared_rij) d_rij = const_cast<double*>(shared_rij);
    else if ((rc = dalloc(h, &d_rij, 9 * (size_t)m))) return rc;
    if ((rc = upload(h, h->d_cum, cum32.data(), (size_t)mp + 1))) return rc;
    if ((rc = upload(h, h->d_pos_edge, s->pos_edge.data(), (size_t)mp))) return rc;
    if ((rc = upload(h, h->d_ejk, s->e_jk.data(), (size_t)mc))) return rc;
    if ((rc = upload(h, h->d_eki, s->e_ki.data(), (size_t)mc))) return rc;
    if ((rc = upload(h, h->d_ikj, s->ikj.data(), (size_t)mc))) return rc;
    if ((rc = upload(h, h->d_jki, s->jki.data(), (size_t)mc))) return rc;
    if ((rc = upload(h, d_k, s->k.data(), (size_t)mc))) return rc;
    if ((rc = upload(h, d_ii, prob->ind_i, (size_t)m))) return rc;
    if ((rc = upload(h, d_jj, prob->ind_j, (size_t)m))) return rc;
    if (!shared_rij && (rc = upload(h, d_rij, prob->rij, 9 * (size_t)m))) return rc;
    DESC_HIP(hipStreamSynchronize(h->stream));
    h->ms_upload = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

    hipEvent_t e0, e1;
    DESC_HIP(hipEventCreate(&e0)); DESC_HIP(hipEventCreate(&e1));
    (void)hipEventRecord(e0, h->stream);
    if (mp > 0) {
        int g = (int)std::min<int64_t>(4096, (mp + 3) / 4);
        hipLaunchKernelGGL(k_cycle_d, dim3(g), dim3(256), 0, h->stream, h->d_cum, h->d_pos_edge, d_ii, d_jj, d_k,
                           h->d_ejk, h->d_eki, d_rij, h->d_S0, (int)mp);
    }
    (void)hipEventRecord(e1, h->stream);
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipGetLastError();
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
    h->ms_cycle_d = ms;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    dfree(h, d_k); dfree(h, d_ii); dfree(h, d_jj); if (!shared_rij) dfree(h, d_rij);
    if (e != hipSuccess) return fail(DESC_ERR_HIP, "k_cycle_d: %s", hipGetErrorString(e));
    return DESC_OK;
}

}  // namespace desc

// The DESC projected-gradient iteration for a caller-supplied step rule (DESC_STEP_EXTERNAL, desc_pgd_ext_*) on gfx950: a gradient pass and an
// apply pass with the caller between them.
// ===========================================================================
// TWO-PHASE iteration: the cut at DESC_PGD.m:207 for a caller-supplied step rule
// ===========================================================================
// params.Gradient may be any object with a GetStep method (:207).  The sweeps (sweep_*.hip) fuse :185-230 into one pass around one of the three known
// rules; here the same iteration is two kernels with the caller between them:
//   gradient pass (:185-204)  mirror-weight sums (node layout: k_colsum_node's fixed-point totals; gather layout: in the kernel), grad_long,
//                             tangent projection -> ONE double per cycle, nothing else written
//   apply pass    (:207-230)  w + step, simplex projection, new S_vec: streams w, step, S0 (24 B read, 8 B written per cycle), no gather of S
// grad_long and the step are in the REFERENCE's cycle order (segment l at cum_ind(l) .. cum_ind(l+1), entries in the order of IJK).  The node
// layout stores segments band-major and the cycles of a segment grouped by mirror class: both kernels index the caller's vector through
// src_start / seg_perm (the tables of k_reorder_cycles), a permutation inside the segment's own contiguous run, so no reorder pass is needed.
// A lane group of G lanes owns a segment, E cycles per lane (cycle q = lane + G e): 16/32/64 x 1 for segments of up to 64 cycles, 64 x 2 and
// 64 x 4 up to 256; reductions = E in-lane adds + group_sum<G>; Michelot's threshold as simplex_threshold<G>.  Longer segments (gather layout
// only): k_ext_grad_big / k_ext_apply_big, one wave per segment in several passes, as k_sweep_big.
#include <algorithm>
#include <cmath>

#include "pgd_handle.h"

namespace desc {

struct ExtArgs {
    const int32_t* cum;          // n_seg + 1, layout order
    const int32_t* src_start;    // node layout: the segment's first cycle in the reference's order
    const uint8_t* seg_perm;     // node layout: reference offset (inside its segment) of the cycle stored at a layout slot
    const EdgeInfo* einfo;       // node layout
    const uint32_t* pk;
    const double* Tfull;
    const int32_t *pos_edge, *e_jk, *e_ki, *ikj, *jki;      // gather layout
    const double *S0, *w_old, *S_old, *nv_tab;
    double *w_new, *S_new;       // apply pass
    double* grad;                // gradient pass: out, reference order
    const double* step;          // apply pass: in, reference order
    double* partials;            // apply pass: [grid][2], slot 1 = sum |dS| (:232)
    double fx_inv;
    int32_t n_seg;
};

template <int G, int E, bool NODE>
__global__ __launch_bounds__(256) void k_ext_grad(ExtArgs a) {
    constexpr int SPW = 64 / G;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sub = lane / G, gl = lane % G;
    for (int l0 = ((int)blockIdx.x * 4 + wv) * SPW; l0 < a.n_seg; l0 += (int)gridDim.x * 4 * SPW) {
        const int l = l0 + sub;
        const bool seg_ok = l < a.n_seg;
        int base = 0, cnt = 0, src = 0;
        EdgeInfo ei{0, 0, 0, 0};
        double T1 = 0.0, T2 = 0.0;
        if (seg_ok) {
            base = a.cum[l]; cnt = a.cum[l + 1] - base; src = base;
            if (NODE) {
                src = a.src_start[l]; ei = a.einfo[l];
                T1 = fx_to_double(a.Tfull[ei.slot_a], a.fx_inv); T2 = fx_to_double(a.Tfull[ei.slot_b], a.fx_inv);
            }
        }
        double ssum[E], d[E]; bool m1[E], m2[E]; int dst[E];
        double wa = 0.0, wb = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int q = gl + G * e;
            const int64_t c = (int64_t)base + q;
            ssum[e] = 0.0; d[e] = 0.0; m1[e] = false; m2[e] = false; dst[e] = -1;
            if (q < cnt) {
                d[e] = a.S0[c];
                if (NODE) {
                    const uint32_t p = a.pk[c];
                    ssum[e] = a.S_old[ei.rb_j + (int)((p >> 16) & 0x7FFFu)] + a.S_old[ei.rb_i + (int)(p & 0x7FFFu)];      // S(jk) + S(ki)
                    m1[e] = (p & 0x8000u) != 0; m2[e] = (p & 0x80000000u) != 0;
                    dst[e] = src + (int)a.seg_perm[c];
                } else {
                    const int ia = a.ikj[c], ib = a.jki[c];
                    ssum[e] = a.S_old[a.e_jk[c]] + a.S_old[a.e_ki[c]];
                    m1[e] = ia >= 0; m2[e] = ib >= 0;
                    if (ia >= 0) wa += a.w_old[ia];
                    if (ib >= 0) wb += a.w_old[ib];
                    dst[e] = src + q;
                }
            }
        }
        if (!NODE) { T1 = group_sum<G>(wa); T2 = group_sum<G>(wb); }                          // :189-190
        const double nv = cnt > 0 ? a.nv_tab[cnt] : 0.0;
        double g[E], dotp = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            g[e] = ssum[e] + ((m1[e] ? T1 : 0.0) + (m2[e] ? T2 : 0.0)) * d[e];                // :193
            dotp += dst[e] >= 0 ? g[e] * nv : 0.0;
        }
        const double dot = group_sum<G>(dotp);                                                // :199-201
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (dst[e] >= 0) a.grad[dst[e]] = g[e] - dot * nv;
    }
}

template <int G, int E, bool NODE>
__global__ __launch_bounds__(256) void k_ext_apply(ExtArgs a) {
    constexpr int SPW = 64 / G;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sub = lane / G, gl = lane % G;
    double chg_acc = 0.0;
    for (int l0 = ((int)blockIdx.x * 4 + wv) * SPW; l0 < a.n_seg; l0 += (int)gridDim.x * 4 * SPW) {
        const int l = l0 + sub;
        const bool seg_ok = l < a.n_seg;
        int base = 0, cnt = 0, src = 0;
        if (seg_ok) { base = a.cum[l]; cnt = a.cum[l + 1] - base; src = NODE ? a.src_start[l] : base; }
        double ws[E], d[E]; bool act[E], on[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int q = gl + G * e;
            const int64_t c = (int64_t)base + q;
            act[e] = q < cnt; ws[e] = 0.0; d[e] = 0.0;
            if (act[e]) {
                ws[e] = a.w_old[c] + a.step[src + (NODE ? (int)a.seg_perm[c] : q)];          // :207
                d[e] = a.S0[c];
            }
            on[e] = act[e];
        }
        double T = 0.0;                                                                       // :215-223 (simplex_threshold, E values per lane)
        for (;;) {
            double s = 0.0; int na = 0;
#pragma unroll
            for (int e = 0; e < E; ++e) { s += on[e] ? ws[e] : 0.0; na += on[e] ? 1 : 0; }
            s = group_sum<G>(s);
            na = E == 1 ? group_count<G>(on[0], lane) : (int)group_sum<G>((double)na);
            T = (s - 1.0) / (double)max(na, 1);
            bool changed = false;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const bool keep = on[e] && (ws[e] > T);
                changed |= keep != on[e];
                on[e] = keep;
            }
            if (!__any(changed)) break;
        }
        double sn = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const double wn = act[e] ? fmax(ws[e] - T, 0.0) : 0.0;                            // :224
            if (act[e]) a.w_new[(int64_t)base + gl + G * e] = wn;
            sn += wn * d[e];
        }
        const double snew = group_sum<G>(sn);                                                 // :229
        if (seg_ok && cnt > 0 && gl == 0) {
            if (NODE) {
                const EdgeInfo ei = a.einfo[l];
                chg_acc += fabs(snew - a.S_old[ei.slot_a]);                                   // :232
                a.S_new[ei.slot_a] = snew; a.S_new[ei.slot_b] = snew;
            } else {
                const int eid = a.pos_edge[l];
                chg_acc += fabs(snew - a.S_old[eid]);
                a.S_new[eid] = snew;
            }
        }
    }
    block_partials(0.0, chg_acc, a.partials, blockIdx.x);
}

// segments longer than 256 cycles (gather layout: the reference's order is the layout's): one wave per segment, several passes; `grad` doubles
// as scratch in the gradient pass and w_new in the apply pass (each lane re-reads only what it wrote itself), as in k_sweep_big
__global__ __launch_bounds__(256) void k_ext_grad_big(ExtArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int l = (int)blockIdx.x * 4 + wv; l < a.n_seg; l += (int)gridDim.x * 4) {
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
            const double g = ssum + ((a.ikj[c] >= 0 ? T1 : 0.0) + (a.jki[c] >= 0 ? T2 : 0.0)) * a.S0[c];
            a.grad[c] = g;
            dotp += g * nv;
        }
        const double dot = group_sum<64>(dotp);
        for (int t = lane; t < cnt; t += 64) {
            const int64_t c = (int64_t)base + t;
            a.grad[c] = a.grad[c] - dot * nv;
        }
    }
}
__global__ __launch_bounds__(256) void k_ext_apply_big(ExtArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double chg_acc = 0.0;
    for (int l = (int)blockIdx.x * 4 + wv; l < a.n_seg; l += (int)gridDim.x * 4) {
        const int base = a.cum[l], cnt = a.cum[l + 1] - base;
        for (int t = lane; t < cnt; t += 64) {
            const int64_t c = (int64_t)base + t;
            a.w_new[c] = a.w_old[c] + a.step[c];
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
            const int eid = a.pos_edge[l];
            chg_acc += fabs(snew - a.S_old[eid]);
            a.S_new[eid] = snew;
        }
    }
    block_partials(0.0, chg_acc, a.partials, blockIdx.x);
}

// Bookkeeping of an applied step (:232-257), one wave: `fc` = the apply pass's partials (sum |dS|), `fo` = the objective kernel's partials
// of the NEW iterate (last_only form: the host sits between two iterations, so the objective is not one sweep late here).
// out = {average_change, objective, stop flag}.
__global__ __launch_bounds__(64) void k_ext_finalize(FinArgs fc, FinArgs fo, double* out) {
    const int lane = threadIdx.x & 63;
    double q0[4], q1[4], r0[4], r1[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) finalize_quarter(fc, w, lane, q0[w], q1[w]);
#pragma unroll
    for (int w = 0; w < 4; ++w) finalize_quarter(fo, w, lane, r0[w], r1[w]);
    if (lane == 0) {
        const double avg = (((q1[0] + q1[1]) + q1[2]) + q1[3]) / (double)fc.m, o = ((r0[0] + r0[1]) + r0[2]) + r0[3];
        fc.avg_trace[fc.t - 1] = avg;                                                         // :232
        finalize_book(fo, o, 0.0);                                                            // :233, :243-256
        out[0] = avg; out[1] = o; out[2] = fo.st->stop ? 1.0 : 0.0;
    }
}

namespace {

enum { EXT_GRAD_DUE = 1, EXT_STEP_DUE = 2, EXT_STOPPED = 3 };

// workgroups of the two passes: four waves of 64 / G segments each per workgroup, grid-stride; the apply pass writes one pair of partials
// per workgroup, so the sweeps' partial buffer bounds it
int ext_grid(const desc_pgd* h, int G) {
    const int64_t per_block = 4 * (G ? 64 / G : 1);
    return (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)parts_cap(h), (h->m_pos + per_block - 1) / per_block));
}
struct ExtShape { int G, E; };      // G = 0: the multi-pass kernels
ExtShape ext_shape(const desc_pgd* h) {
    const int c = h->max_cnt;
    if (c <= 16) return {16, 1};
    if (c <= 32) return {32, 1};
    if (c <= 64) return {64, 1};
    if (c <= 128) return {64, 2};
    if (c <= 256) return {64, 4};
    return {0, 0};
}
ExtArgs ext_args(const desc_pgd* h, int rd, int wr) {
    ExtArgs a{};
    a.cum = h->d_cum; a.S0 = h->d_S0; a.w_old = h->d_w[rd]; a.w_new = h->d_w[wr]; a.S_old = h->d_S[rd]; a.S_new = h->d_S[wr];
    a.nv_tab = h->d_nv; a.partials = h->d_partials; a.n_seg = (int32_t)h->m_pos;
    if (h->variant == VARIANT_NODE) {
        a.src_start = h->d_src_start; a.seg_perm = h->d_seg_perm; a.einfo = h->d_einfo; a.pk = h->d_pk; a.Tfull = h->d_T;
        a.fx_inv = std::ldexp(1.0, -h->colsum_fx_bits);
    } else {
        a.pos_edge = h->d_pos_edge; a.e_jk = h->d_ejk; a.e_ki = h->d_eki; a.ikj = h->d_ikj; a.jki = h->d_jki;
    }
    return a;
}
template <bool NODE>
void launch_ext(desc_pgd* h, const ExtArgs& a, bool apply) {
    const ExtShape sh = ext_shape(h);
    const dim3 grid(ext_grid(h, sh.G)), block(256);
#define DESC_EXT_CASE(G_, E_)                                                                             \
    case G_ * 8 + E_:                                                                                     \
        if (apply) hipLaunchKernelGGL((k_ext_apply<G_, E_, NODE>), grid, block, 0, h->stream, a);         \
        else hipLaunchKernelGGL((k_ext_grad<G_, E_, NODE>), grid, block, 0, h->stream, a);                \
        break;
    switch (sh.G * 8 + sh.E) {
        DESC_EXT_CASE(16, 1) DESC_EXT_CASE(32, 1) DESC_EXT_CASE(64, 1) DESC_EXT_CASE(64, 2) DESC_EXT_CASE(64, 4)
        default:
            if (apply) hipLaunchKernelGGL(k_ext_apply_big, grid, block, 0, h->stream, a);
            else hipLaunchKernelGGL(k_ext_grad_big, grid, block, 0, h->stream, a);
            break;
    }
#undef DESC_EXT_CASE
}
int ext_check(const desc_pgd* h, const char* what) {
    if (h->world > 1) return fail(DESC_ERR_STATE, "%s: a sharded handle (world %d) cannot run a caller-supplied step rule", what, h->world);
    return DESC_OK;
}
int ext_check_where(int32_t where) {
    if (where != DESC_MEM_HOST && where != DESC_MEM_DEVICE) return fail(DESC_ERR_INVALID, "where must be DESC_MEM_HOST or DESC_MEM_DEVICE");
    return DESC_OK;
}

}  // namespace

}  // namespace desc

using namespace desc;

extern "C" {

int desc_pgd_ext_begin(desc_pgd* h, const desc_params* p) {
    if (!h || !p) return fail(DESC_ERR_INVALID, "NULL argument");
    int rc = ext_check(h, "desc_pgd_ext_begin"); if (rc) return rc;
    if (p->step_kind != DESC_STEP_EXTERNAL) return fail(DESC_ERR_INVALID, "desc_pgd_ext_begin: params.step_kind must be DESC_STEP_EXTERNAL (is %d)", p->step_kind);
    desc_params q = *p;
    q.step_kind = DESC_STEP_CONSTANT;                    // :148-180 do not depend on the step rule
    if ((rc = desc_pgd_reset(h, &q))) return rc;
    h->p.step_kind = DESC_STEP_EXTERNAL;
    if (h->m_cycle > 0 && !h->d_ext_io && (rc = dalloc(h, &h->d_ext_io, (size_t)h->m_cycle))) return rc;
    if (!h->d_ext_out && (rc = dalloc(h, &h->d_ext_out, 4))) return rc;
    for (auto& e : h->ev_ext) if (!e) DESC_HIP(hipEventCreate(&e));
    h->ext_ms[0] = h->ext_ms[1] = h->ext_ms[2] = 0.0;
    DESC_HIP(hipStreamSynchronize(h->stream));
    h->ext_phase = EXT_GRAD_DUE;
    return DESC_OK;
}

int desc_pgd_ext_grad(desc_pgd* h, double* grad_long, int32_t where) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    int rc = ext_check(h, "desc_pgd_ext_grad"); if (rc) return rc;
    if (!h->ext_phase) return fail(DESC_ERR_STATE, "desc_pgd_ext_grad: desc_pgd_ext_begin must be called first");
    if (h->ext_phase == EXT_STOPPED) return fail(DESC_ERR_STATE, "desc_pgd_ext_grad: the stop rule (DESC_PGD.m:243-246) has fired at iteration %d", h->t_done);
    if (h->t_done >= h->iters_cap) return fail(DESC_ERR_STATE, "desc_pgd_ext_grad: params.iters = %d steps have been applied", h->p.iters);
    if ((rc = ext_check_where(where))) return rc;
    if (!grad_long && h->m_cycle > 0) return fail(DESC_ERR_INVALID, "grad_long is NULL");
    if ((rc = set_device(h))) return rc;
    if (h->m_pos > 0) {
        const int rd = h->t_done & 1;
        ExtArgs a = ext_args(h, rd, rd ^ 1);
        a.grad = where == DESC_MEM_DEVICE ? grad_long : h->d_ext_io;
        DESC_HIP(hipEventRecord(h->ev_ext[0], h->stream));
        if (h->variant == VARIANT_NODE) {
            FinArgs none{}; none.st = nullptr;                                                  // no sweep's bookkeeping rides on this launch
            launch_colsum(h, h->stream, h->d_w[rd], h->d_T, nullptr, none);                     // :185-191
            launch_ext<true>(h, a, false);
        } else
            launch_ext<false>(h, a, false);
        DESC_HIP(hipEventRecord(h->ev_ext[1], h->stream));
        DESC_HIP(hipGetLastError());
        DESC_HIP(hipStreamSynchronize(h->stream));
        float ms = 0; DESC_HIP(hipEventElapsedTime(&ms, h->ev_ext[0], h->ev_ext[1]));
        h->ext_ms[0] = ms; h->ms_pgd += ms;
        if (where == DESC_MEM_HOST) DESC_HIP(hipMemcpy(grad_long, h->d_ext_io, sizeof(double) * h->m_cycle, hipMemcpyDeviceToHost));
    }
    h->ext_phase = EXT_STEP_DUE;
    return DESC_OK;
}

int desc_pgd_ext_apply(desc_pgd* h, const double* step, int32_t where, double* average_change, double* objective, int32_t* stopped) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    int rc = ext_check(h, "desc_pgd_ext_apply"); if (rc) return rc;
    if (!h->ext_phase) return fail(DESC_ERR_STATE, "desc_pgd_ext_apply: desc_pgd_ext_begin must be called first");
    if (h->ext_phase == EXT_STOPPED) return fail(DESC_ERR_STATE, "desc_pgd_ext_apply: the stop rule (DESC_PGD.m:243-246) has fired at iteration %d", h->t_done);
    if (h->ext_phase != EXT_STEP_DUE) return fail(DESC_ERR_STATE, "desc_pgd_ext_apply: no gradient has been handed out for this iteration (call desc_pgd_ext_grad first)");
    if ((rc = ext_check_where(where))) return rc;
    if (!step && h->m_cycle > 0) return fail(DESC_ERR_INVALID, "step is NULL");
    if ((rc = set_device(h))) return rc;
    const int t = h->t_done + 1;
    double out[3] = {0.0, 0.0, 0.0};
    if (h->m_pos > 0) {
        const int rd = (t - 1) & 1, wr = t & 1;
        ExtArgs a = ext_args(h, rd, wr);
        if (where == DESC_MEM_HOST) {
            DESC_HIP(hipMemcpyAsync(h->d_ext_io, step, sizeof(double) * h->m_cycle, hipMemcpyHostToDevice, h->stream));
            a.step = h->d_ext_io;
        } else
            a.step = step;
        DESC_HIP(hipEventRecord(h->ev_ext[2], h->stream));
        const ExtShape sh = ext_shape(h);
        if (h->variant == VARIANT_NODE) launch_ext<true>(h, a, true); else launch_ext<false>(h, a, true);
        DESC_HIP(hipEventRecord(h->ev_ext[3], h->stream));
        // :232-257 for this iteration, at once: the objective of the new iterate, the traces and the patience test
        launch_objective(h, h->stream, wr, h->obj_grid, obj_partials(h));
        hipLaunchKernelGGL(k_ext_finalize, dim3(1), dim3(64), 0, h->stream, fin_args(h, h->d_partials, ext_grid(h, sh.G), t, 0), fin_args(h, obj_partials(h), h->obj_grid, t, 1),
                           h->d_ext_out);
        DESC_HIP(hipEventRecord(h->ev_ext[4], h->stream));
        DESC_HIP(hipGetLastError());
        DESC_HIP(hipStreamSynchronize(h->stream));
        DESC_HIP(hipMemcpy(out, h->d_ext_out, sizeof out, hipMemcpyDeviceToHost));
        float ms1 = 0, ms2 = 0;
        DESC_HIP(hipEventElapsedTime(&ms1, h->ev_ext[2], h->ev_ext[3]));
        DESC_HIP(hipEventElapsedTime(&ms2, h->ev_ext[3], h->ev_ext[4]));
        h->ext_ms[1] = ms1; h->ext_ms[2] = ms2; h->ms_pgd += ms1 + ms2;
        h->final_obj_T = t;                              // desc_pgd_download: this iterate's objective and stop test are done
    } else if (t >= h->p.patience + 1)
        out[2] = 1.0;                                    // no cycle at all: objective 0 for ever, `patience` misses counted from iteration 2
    h->t_done = t; h->t_plugin += 1;
    h->ext_phase = out[2] != 0.0 ? EXT_STOPPED : EXT_GRAD_DUE;
    if (average_change) *average_change = out[0];
    if (objective) *objective = out[1];
    if (stopped) *stopped = out[2] != 0.0 ? 1 : 0;
    return DESC_OK;
}

int desc_pgd_ext_laps(const desc_pgd* h, double* ms3) {
    if (!h || !ms3) return fail(DESC_ERR_INVALID, "NULL argument");
    for (int q = 0; q < 3; ++q) ms3[q] = h->ext_ms[q];
    return DESC_OK;
}

}  // extern "C"

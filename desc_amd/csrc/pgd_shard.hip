// The multi-GPU protocol of the DESC projected-gradient solver (node layout, gfx950): the pieces of a sharded iteration -- column sums into the
// exchange layout, the sweep of the owned segments, the unpacking of the gathered S -- as separate entry points (the caller runs the collectives
// between them), and the fused protocol that enqueues whole iterations from C with the exchange on a second stream.  The exchange layout itself
// (k_xpos, k_xt, k_prefB, k_node_runs) is made by setup_node (pgd_layout.hip).
#include <algorithm>
#include <chrono>

#include "pgd_handle.h"

namespace desc {

namespace {

// the pieces of one sharded iteration, each enqueued on the stream given
// One rank and nothing forcing the exchange layout: the column sums stay in CSR order (coalesced row writes) exactly as in
// the unsharded path.  With more ranks every rank writes all 2m slots of the owner-sorted layout, 8 bytes at a time
// (measured at C4: +74 us on the column-sum pass, independent of the number of ranks).
bool shard_direct(const desc_pgd* h) { return h->world == 1 && !h->force_coll && h->comm_stream != nullptr; }
int shard_enqueue_colsum(desc_pgd* h, hipStream_t st) {
    const int rd = h->t_done & 1;
    const bool direct = shard_direct(h);
    launch_colsum(h, st, h->d_w[rd], direct ? h->d_T : h->x_T, direct ? nullptr : h->d_xpos, FinArgs{});
    DESC_HIP(hipGetLastError());
    return DESC_OK;
}
double* my_slice(desc_pgd* h) { return h->x_sall + (int64_t)h->rank * h->slice_len; }
// sweep number t of the exchange parts [part_lo, part_hi): one launch each (part c reads the sums of ITS reduce-scatter: x_Trecv + c * t_part).
// first: this call opens sweep t (plugin step, iteration counter); the parts of one sweep share the step.
int shard_enqueue_sweep(desc_pgd* h, hipStream_t st, int part_lo = 0, int part_hi = -1) {
    if (part_hi < 0) part_hi = h->xparts;
    const bool first = part_lo == 0;
    if (first && h->t_done + 1 > h->iters_cap) return fail(DESC_ERR_INVALID, "iterating past params.iters = %d", h->p.iters);
    if (first) { ++h->t_done; h->cur_step = make_step(h, &h->cur_adam, (h->t_done - 1) & 1, h->t_done & 1); }
    const int t = h->t_done, rd = (t - 1) & 1, wr = t & 1;
    const bool adam = h->cur_adam;
    // a handle on the band sweep runs its parts as separate launches; k_sweep_node (tiny graphs, Adam on long segments) has one part
    const bool by_parts = adam ? band_adam_ok(h) : h->band_ok;
    for (int c = part_lo; c < part_hi; ++c) {
        if (!by_parts && c > 0) break;
        NodeSweepArgs a = node_sweep_args(h, rd, wr);
        a.st = h->cur_step; a.xt = h->d_xt;
        a.Tfull = h->x_Trecv + (int64_t)c * h->t_part;
        // S and the workgroup partials go straight into the slice: the part's S behind the parts before it, its partials in its share of the partial area
        a.s_slice = my_slice(h) + h->xslice_off[c];
        a.partials = my_slice(h) + h->slice_S + 2 * (int64_t)c * (SHARD_PARTS / h->xparts);
        a.t_bytes = (uint32_t)(8 * h->t_part); a.slice_bytes = (uint32_t)(8 * (h->slice_S - h->xslice_off[c]));
        if (shard_direct(h)) { a.Tfull = h->d_T; a.xt = nullptr; a.s_slice = nullptr; a.t_bytes = a.csr_bytes; }
        const hipStream_t keep = h->stream; h->stream = st;
        const int rc = launch_sweep_node_layout(h, a, adam, c);
        h->stream = keep;
        if (rc) return rc;
    }
    h->last_parts = sweep_parts(h, adam);
    DESC_HIP(hipGetLastError());
    return DESC_OK;
}
// after the all-gather: S of every edge into the CSR-aligned copy (+ traces and stop rule of sweep t when fin_t > 0)
int shard_enqueue_unpack(desc_pgd* h, hipStream_t st, double* S_a, double* S_b, int fin_t, int last_only, int /*nparts*/) {
    const int g = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (2 * h->m + 255) / 256));
    // the whole partial area of every slice is added (sweep grids may differ between ranks on tiny problems; unused pairs are zero)
    FinArgs f = fin_args(h, h->x_sall + h->slice_S, SHARD_PARTS, fin_t, last_only);
    f.rank_stride = h->slice_len; f.nranks = h->world;
    launch_unpack(h, st, g, S_a, S_b, f);
    if (last_only)        // the objective pass filled more pairs than a sweep does: clear this rank's area for further iterations
        DESC_HIP(hipMemsetAsync(my_slice(h) + h->slice_S, 0, sizeof(double) * 2 * SHARD_PARTS, st));
    DESC_HIP(hipGetLastError());
    return DESC_OK;
}
int shard_enqueue_objective(desc_pgd* h, hipStream_t st) {
    // exactly SHARD_PARTS workgroups on every rank (idle ones write zeros): the partial areas of all slices are summed in full
    launch_objective(h, st, h->t_done & 1, SHARD_PARTS, my_slice(h) + h->slice_S);
    DESC_HIP(hipGetLastError());
    return DESC_OK;
}
int coll_fail(int code, const char* what) { return fail(DESC_ERR_HIP, "%s failed with code %d", what, code); }
int shard_all_gather(desc_pgd* h) {
    if (h->world == 1 && !h->force_coll) return DESC_OK;
    const int rcc = h->coll.all_gather(my_slice(h), h->x_sall, (size_t)h->slice_len, 8 /* ncclDouble */, h->coll.comm, h->comm_stream);
    return rcc ? coll_fail(rcc, "all_gather") : DESC_OK;
}

}  // namespace

// the all-gather of sweep t has been enqueued on the exchange stream (ev_ag behind it): its unpacking + the stop rule, on the compute stream
int shard_unpack_pending(desc_pgd* h) {
    if (!h->unpack_pending) return DESC_OK;
    const int t = h->unpack_pending;
    h->unpack_pending = 0;
    DESC_HIP(hipStreamWaitEvent(h->stream, h->ev_ag, 0));
    // one rank on the direct path: the sweep already wrote S of every edge; only the bookkeeping is left
    return shard_enqueue_unpack(h, h->stream, shard_direct(h) ? nullptr : h->d_S[t & 1], nullptr, t, 0, h->last_parts);
}

}  // namespace desc

using namespace desc;

extern "C" {

// ------------------------------------------------------------- multi-GPU pieces --
int desc_pgd_shard_info(const desc_pgd* h, desc_shard_info* info) {
    if (!h || !info) return fail(DESC_ERR_INVALID, "NULL argument");
    info->rank = h->rank; info->world = h->world;
    info->t_len = (int64_t)h->world * h->xparts * h->t_part + 1; info->t_part = h->t_part; info->slice_len = h->slice_len; info->xparts = h->xparts;
    info->seg_lo = h->seg_lo; info->seg_hi = h->seg_hi; info->cyc_lo = h->cyc_lo; info->cyc_hi = h->cyc_hi;
    info->m_pos = h->m_pos; info->m_cycle = h->m_cycle;
    return DESC_OK;
}

int desc_pgd_shard_bind(desc_pgd* h, double* T_send, double* T_recv, double* sall, void* hip_stream) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    if (h->variant != VARIANT_NODE) return fail(DESC_ERR_STATE, "sharding needs the node layout");
    int rc = set_device(h); if (rc) return rc;
    DESC_HIP(hipStreamSynchronize(h->stream));
    if (sweep_parts(h, false) > SHARD_PARTS || h->grid > SHARD_PARTS) return fail(DESC_ERR_STATE, "sweep grid exceeds the partials area of the exchange slice");
    // every exchange part's band sweep writes band_grid + its tail pairs into its own share of the partials area (shard_enqueue_sweep)
    if (h->band_ok)
        for (int c = 0; c < h->xparts; ++c)
            if (h->band_grid + h->xntail[c] > SHARD_PARTS / h->xparts)
                return fail(DESC_ERR_STATE, "exchange part %d: %d sweep workgroups + %d tail pieces exceed its %d partial pairs", c, h->band_grid, h->xntail[c],
                            SHARD_PARTS / h->xparts);
    if (!T_send && !T_recv && !sall) {       // library-owned exchange buffers (the fused protocol does not need torch tensors)
        const int64_t t_len = (int64_t)h->world * h->xparts * h->t_part + 1;
        if ((rc = dalloc(h, &T_send, (size_t)t_len))) return rc;
        if (h->world > 1) { if ((rc = dalloc(h, &T_recv, (size_t)h->xparts * h->t_part))) return rc; }
        else T_recv = T_send;                // one rank: the owner-sorted partial sums ARE the totals
        if ((rc = dalloc(h, &sall, (size_t)(h->world * h->slice_len)))) return rc;
        DESC_HIP(hipMemsetAsync(T_send, 0, sizeof(double) * t_len, h->stream));
        DESC_HIP(hipMemsetAsync(sall, 0, sizeof(double) * h->world * h->slice_len, h->stream));
        DESC_HIP(hipStreamSynchronize(h->stream));
        h->own_xbuf = true;
    } else if (!T_send || !T_recv || !sall) return fail(DESC_ERR_INVALID, "NULL exchange buffer");
    h->x_T = T_send; h->x_Trecv = T_recv; h->x_sall = sall;
    if (hip_stream) {          // run on the caller's stream so collectives and kernels are ordered
        if (h->stream) { (void)hipStreamSynchronize(h->stream); stream_release(h->stream); }
        h->stream = (hipStream_t)hip_stream;
        h->borrowed_stream = true;
    }
    return DESC_OK;
}

// step 1 of an iteration: partial column sums of the segments this rank owns -> T_send, grouped by the
// rank that owns each edge (then: reduce-scatter(sum) T_send -> T_recv)
int desc_pgd_shard_colsum(desc_pgd* h) {
    if (!h || !h->armed || !h->x_T) return fail(DESC_ERR_STATE, "shard not armed / bound");
    int rc = set_device(h); if (rc) return rc;
    return shard_enqueue_colsum(h, h->stream);
}

// step 2: sweep the owned chunks (T_recv holds the global sums); S of the owned edges and the workgroup partials
// are written straight into this rank's slice of sall (then: all-gather sall)
int desc_pgd_shard_sweep(desc_pgd* h) {
    if (!h || !h->armed || !h->x_T) return fail(DESC_ERR_STATE, "shard not armed / bound");
    int rc = set_device(h); if (rc) return rc;
    return shard_enqueue_sweep(h, h->stream);
}

// step 3: (sall gathered) scatter S of every edge into the CSR-aligned copy, add the partials of all ranks in
// rank order, record traces, early-stop rule.
// initial: 1 = after desc_pgd_reset, before the first all-gather (the reset already put the initial S of the owned
// edges into the slice: nothing to do); 2 = after that all-gather: distribute the initial S_vec, no traces.
int desc_pgd_shard_finish(desc_pgd* h, int32_t initial) {
    if (!h || !h->armed || !h->x_sall) return fail(DESC_ERR_STATE, "shard not armed / bound");
    int rc = set_device(h); if (rc) return rc;
    const int t = h->t_done, wr = t & 1;
    if (initial && t != 0) return fail(DESC_ERR_STATE, "initial exchange after iterations");
    if (initial == 1) return DESC_OK;
    if (initial == 2) return shard_enqueue_unpack(h, h->stream, h->d_S[0], h->d_S[1], 0, 0, 0);
    return shard_enqueue_unpack(h, h->stream, h->d_S[wr], nullptr, t, 0, h->last_parts);
}

// final objective of a sharded run: phase 0 puts this rank's partials into its slice (then: all-gather sall),
// phase 1 adds the partials of all ranks and runs the stop rule for the last iteration.
int desc_pgd_shard_objective(desc_pgd* h, int32_t phase) {
    if (!h || !h->armed || !h->x_sall) return fail(DESC_ERR_STATE, "shard not armed / bound");
    int rc = set_device(h); if (rc) return rc;
    const int T = h->t_done;
    if (T < 1) return DESC_OK;
    if (phase == 0) return shard_enqueue_objective(h, h->stream);
    rc = shard_enqueue_unpack(h, h->stream, nullptr, nullptr, T, 1, h->obj_grid);
    h->objective_done = true; h->final_obj_T = T;
    return rc;
}

// ---- the fused protocol: whole iterations enqueued from C, exchange overlapped with the next column-sum pass
int desc_pgd_shard_set_collectives(desc_pgd* h, const desc_collectives* c) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    if (h->variant != VARIANT_NODE) return fail(DESC_ERR_STATE, "sharding needs the node layout");
    if (h->world > 1 && (!c || !c->reduce_scatter || !c->all_gather)) return fail(DESC_ERR_INVALID, "world > 1 needs both collectives");
    int rc = set_device(h); if (rc) return rc;
    h->coll = c ? *c : desc_collectives{};
    // diagnostics: call the collectives even with one rank (plumbing test of the RCCL entry points on a one-GPU box)
    h->force_coll = env_int("DESC_DEBUG_FORCE_COLLECTIVES", 0) != 0 && h->coll.reduce_scatter && h->coll.all_gather;
    if (!h->x_sall && (rc = desc_pgd_shard_bind(h, nullptr, nullptr, nullptr, nullptr))) return rc;
    if (!h->comm_stream) {
        DESC_HIP(stream_acquire(&h->comm_stream));
        for (hipEvent_t* e : {&h->ev_col, &h->ev_rs, &h->ev_sw, &h->ev_ag}) DESC_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
        for (int c = 0; c < 8; ++c) DESC_HIP(hipEventCreateWithFlags(&h->ev_rsx[c], hipEventDisableTiming));
    }
    return DESC_OK;
}

// reset + the initial exchange (every rank ends up with the full initial S_vec)
int desc_pgd_shard_start(desc_pgd* h, const desc_params* p) {
    if (!h || !p) return fail(DESC_ERR_INVALID, "NULL argument");
    if (!h->comm_stream) return fail(DESC_ERR_STATE, "desc_pgd_shard_set_collectives must be called first");
    int rc = desc_pgd_reset(h, p); if (rc) return rc;
    DESC_HIP(hipEventRecord(h->ev_sw, h->stream));
    DESC_HIP(hipStreamWaitEvent(h->comm_stream, h->ev_sw, 0));
    if ((rc = shard_all_gather(h))) return rc;
    DESC_HIP(hipEventRecord(h->ev_ag, h->comm_stream));
    DESC_HIP(hipStreamWaitEvent(h->stream, h->ev_ag, 0));
    if ((rc = shard_enqueue_unpack(h, h->stream, h->d_S[0], h->d_S[1], 0, 0, 0))) return rc;
    h->unpack_pending = 0;
    return DESC_OK;
}

// n iterations (round 4):
//   compute stream   colsum(t+1) | unpack(t) + stop rule | sweep(t+1)
//   exchange stream  AG(t)       | RS(t+1) . . . . . . . |            AG(t+1)
// colsum(t+1) needs only the weights of sweep t: it runs under the all-gather of S(t); the unpacking of S(t) runs under the reduce-scatter
// of the mirror sums.  (Round 3 had the unpack on the exchange stream IN FRONT of the reduce-scatter: measured per rank of 8 at C4,
// profiles/r04_shard_w8_c4_*.json, all-gather + unpack (~60 + 90 us) outlast the column sums (50-80 us), so the reduce-scatter started late.)
int desc_pgd_shard_iterate(desc_pgd* h, int32_t n_iters) {
    if (!h || !h->armed) return fail(DESC_ERR_STATE, "desc_pgd_shard_start must be called first");
    if (!h->comm_stream) return fail(DESC_ERR_STATE, "desc_pgd_shard_set_collectives must be called first");
    if (n_iters < 0 || h->t_done + n_iters > h->iters_cap) return fail(DESC_ERR_INVALID, "iterating past params.iters = %d", h->p.iters);
    int rc = set_device(h); if (rc) return rc;
    for (int q = 0; q < n_iters; ++q) {
        if ((rc = shard_enqueue_colsum(h, h->stream))) return rc;
        const bool exchange = h->world > 1 || h->force_coll;
        if (exchange) {
            DESC_HIP(hipEventRecord(h->ev_col, h->stream));
            DESC_HIP(hipStreamWaitEvent(h->comm_stream, h->ev_col, 0));
            for (int c = 0; c < h->xparts; ++c) {                          // part c: blocks [c * world, (c + 1) * world) of the send buffer
                const int rcc = h->coll.reduce_scatter(h->x_T + (int64_t)c * h->world * h->t_part, h->x_Trecv + (int64_t)c * h->t_part, (size_t)h->t_part,
                                                       4 /* ncclInt64: fixed-point mirror sums, order-independent */, 0 /* ncclSum */, h->coll.comm, h->comm_stream);
                if (rcc) return coll_fail(rcc, "reduce_scatter");
                DESC_HIP(hipEventRecord(h->ev_rsx[c], h->comm_stream));
            }
        }
        if ((rc = shard_unpack_pending(h))) return rc;                  // S of the previous sweep into the CSR-aligned replica, under the reduce-scatter
        for (int c = 0; c < h->xparts; ++c) {                           // part c is swept while part c + 1 is still on the wire
            if (exchange) DESC_HIP(hipStreamWaitEvent(h->stream, h->ev_rsx[c], 0));
            if ((rc = shard_enqueue_sweep(h, h->stream, c, c + 1))) return rc;
        }
        DESC_HIP(hipEventRecord(h->ev_sw, h->stream));
        DESC_HIP(hipStreamWaitEvent(h->comm_stream, h->ev_sw, 0));
        if ((rc = shard_all_gather(h))) return rc;
        DESC_HIP(hipEventRecord(h->ev_ag, h->comm_stream));
        h->unpack_pending = h->t_done;
    }
    return DESC_OK;
}

// start + iterate (polling the stop flag every check_every iterations) + final objective + download
int desc_pgd_shard_run(desc_pgd* h, const desc_params* p, desc_result* r) {
    if (!h || !p || !r) return fail(DESC_ERR_INVALID, "NULL argument");
    auto t0 = std::chrono::steady_clock::now();
    int rc = desc_pgd_shard_start(h, p); if (rc) return rc;
    const int chunk = p->check_every > 0 ? p->check_every : 32;
    int left = p->iters;
    while (left > 0) {
        const int nq = std::min(left, chunk);
        if ((rc = desc_pgd_shard_iterate(h, nq))) return rc;
        left -= nq;
        if (left > 0) { int32_t stop = 0; if ((rc = desc_pgd_stopped(h, &stop))) return rc; if (stop) break; }
    }
    if (h->t_done >= 1) {
        if ((rc = shard_unpack_pending(h))) return rc;
        if ((rc = shard_enqueue_objective(h, h->stream))) return rc;
        DESC_HIP(hipEventRecord(h->ev_sw, h->stream));
        DESC_HIP(hipStreamWaitEvent(h->comm_stream, h->ev_sw, 0));
        if ((rc = shard_all_gather(h))) return rc;
        DESC_HIP(hipEventRecord(h->ev_ag, h->comm_stream));
        DESC_HIP(hipStreamWaitEvent(h->stream, h->ev_ag, 0));
        if ((rc = shard_enqueue_unpack(h, h->stream, nullptr, nullptr, h->t_done, 1, h->obj_grid))) return rc;
        h->objective_done = true; h->final_obj_T = h->t_done;
    }
    rc = desc_pgd_download(h, r); if (rc) return rc;
    r->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return DESC_OK;
}

// Diagnostics (tests/test_gpu_sharded.py): the exchange layout of a sharded handle.  xpos, spos: 2m entries each (CSR slot -> place of its
// column sum in the reduce-scatter send buffer / place of its edge's S in the gathered slices); xt: 2 * (seg_hi - seg_lo) entries, {ta, tb}
// of the owned segments in device order; slot_ab: the same count, {slot_a, slot_b} = the CSR slots of those segments' edges.
int desc_debug_shard_layout(desc_pgd* h, int32_t* xpos, int32_t* spos, int32_t* xt, int32_t* slot_ab) {
    return no_throw("desc_debug_shard_layout", [&]() -> int {
    if (!h || !xpos || !spos || !xt || !slot_ab) return fail(DESC_ERR_INVALID, "NULL argument");
    if (h->variant != VARIANT_NODE) return fail(DESC_ERR_STATE, "sharding needs the node layout");
    int rc = set_device(h); if (rc) return rc;
    DESC_HIP(hipStreamSynchronize(h->stream));
    if (h->m > 0) {
        DESC_HIP(hipMemcpy(xpos, h->d_xpos, sizeof(int32_t) * 2 * (size_t)h->m, hipMemcpyDeviceToHost));
        DESC_HIP(hipMemcpy(spos, h->d_spos, sizeof(int32_t) * 2 * (size_t)h->m, hipMemcpyDeviceToHost));
    }
    const int64_t nsl = h->seg_hi - h->seg_lo;
    if (nsl > 0) {
        DESC_HIP(hipMemcpy(xt, h->d_xt + h->seg_lo, sizeof(int2) * (size_t)nsl, hipMemcpyDeviceToHost));
        hvec<EdgeInfo> ei((size_t)nsl);
        DESC_HIP(hipMemcpy(ei.data(), h->d_einfo + h->seg_lo, sizeof(EdgeInfo) * (size_t)nsl, hipMemcpyDeviceToHost));
        for (int64_t q = 0; q < nsl; ++q) { slot_ab[2 * q] = ei[q].slot_a; slot_ab[2 * q + 1] = ei[q].slot_b; }
    }
    return DESC_OK;
    });
}

}  // extern "C"

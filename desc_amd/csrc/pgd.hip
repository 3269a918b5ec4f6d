// HIP kernels and solver handle for the DESC projected-gradient hot path on gfx950.
//
// Reference text reproduced (Algorithms/DESC_PGD.m, identical in DESC.m:16-261):
//   :129-147  cycle inconsistency S0_long = |acos((tr(Rij Rjk Rki)-1)/2)|/pi
//   :148-157  wijk = 1/cnt, S_vec = 1 / segment mean of S0
//   :185-191  mirror-weight sums (scalar per edge, broadcast to masked positions)
//   :193-207  gradient, tangent projection, plugin step (Utils/ConstantStepSize.m:9-11,
//             PiecewiseStepSize.m:13-18, HybridGradient.m:23-41)
//   :208-230  per-edge simplex projection, new S_vec
//   :232-257  average_change, objective, early stop (evaluated on the device)
// and, for a params.Gradient object that is none of the three classes (:207 calls GetStep on any handle object), the same
// iteration cut at :207 into a gradient pass and an apply pass with the caller between them (TWO-PHASE iteration, desc_pgd_ext_*).
//
// The NODE layout (default) and the GATHER fallback are described in pgd_layout.hip.  On the node layout the mirror sums are column
// sums of per-node weight matrices: T1(i,j) = sum_k w(ik;j) = column j of node i, T2(i,j) = column i of node j.  k_colsum_node streams,
// per endpoint, the cycles of every incident segment whose mirror was sampled and accumulates the columns in LDS (per-wave private
// copies, fixed order -> bitwise reproducible); k_sweep_node then needs no gather of w at all.
//
// The objective of iteration t needs S_vec of every edge after iteration t, so it
// cannot be fused into sweep t; it is accumulated for free inside sweep t+1 (which
// gathers exactly those values) and once more by an objective kernel after the last
// sweep.  The early-stop test of iteration t is therefore evaluated on the device
// during sweep t+1; when it fires, sweep t+1's output is discarded (the Jacobi double
// buffers still hold iteration t) and later launches return at once.
//
// Units of the PGD solver (struct desc_pgd and what crosses units: pgd_handle.h, host; pgd_device.h and pgd_math.h, device; node_plan.h):
//   pgd.hip            this file: the handle's life cycle, reset, the one-rank run loop, download and the small kernels they launch; the column-sum pass
//                      (k_colsum_node) and k_unpack_S of the sharded runs, which share finalize_quarter with k_finalize (see k_finalize)
//   pgd_layout.hip     the node layout: its description, the kernels that build it, setup_node
//   pgd_shard.hip      the multi-GPU protocol (desc_pgd_shard_*)
//   pgd_ext.hip        the two-phase iteration for caller-supplied step rules (desc_pgd_ext_*)
//   sweep_gather.hip, sweep_node.hip, sweep_band.hip      the three sweep families: kernels, instance table and launcher each
//   node_plan.cpp      the host-side plan of the node layout (no device call)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "pgd_handle.h"

namespace desc {

__global__ __launch_bounds__(256) void k_objective(const double* w, const double* S, const int32_t* e_jk,
                                                   const int32_t* e_ki, int64_t m_cycle, double* partials,
                                                   const DevState* st) {
    if (st->stop) return;
    double acc = 0.0;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < m_cycle; c += (int64_t)gridDim.x * 256)
        acc += w[c] * (S[e_jk[c]] + S[e_ki[c]]);
    block_partials(acc, 0.0, partials, blockIdx.x);
}

// wijk = 1/cnt, S_vec(IJ) = wijk_seg * S0_seg'  (DESC_PGD.m:151-157); one wave per edge
__global__ __launch_bounds__(256) void k_init(const int32_t* cum, const int32_t* pos_edge, const double* S0,
                                              double* w, double* S_a, double* S_b, int m_pos) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t l = wid; l < m_pos; l += nw) {
        const int base = cum[l], cnt = cum[l + 1] - base;
        const double w0 = 1.0 / (double)cnt;
        double s = 0.0;
        for (int t = lane; t < cnt; t += 64) { w[(int64_t)base + t] = w0; s += w0 * S0[(int64_t)base + t]; }
        s = group_sum<64>(s);
        if (lane == 0) { S_a[pos_edge[l]] = s; S_b[pos_edge[l]] = s; }
    }
}

// The bookkeeping of a sweep (pgd_device.h) as a launch of its own, when no column-sum launch is there to carry it.  k_colsum_node and k_unpack_S
// stay in this unit with it: alone in a unit, finalize_block is the only caller of finalize_quarter, the compiler then knows the range of its
// `quarter` argument (wv = threadIdx.x >> 6) and emits other code for the three kernels (44 bytes more each) than next to finalize_wave's loop.
__global__ __launch_bounds__(64) void k_finalize(FinArgs f) { finalize_wave(f); }

// Mirror-weight column sums (DESC_PGD.m:185-191 in node form).  One workgroup per node
// v: for every incident edge {v,u} (CSR order) stream its segment; a cycle with third
// vertex t adds its weight to column idx_v(t) if the reverse cycle ({v,t};u) was sampled.
// Each wave owns a private copy of the columns in LDS (segments are dealt to waves
// round-robin; third vertices inside a segment are distinct), copies are added in a
// fixed order at the end -> bitwise reproducible.  Loads of COLSUM_U segments are in
// flight per wave at once.
// Round 3, what bounds it (profiles/r03_colsum_bound.txt): with the LDS adds replaced by plain stores or removed altogether the kernel takes
// 227.3 / 224.7 us instead of 227.0 at C4 -- the adds are free, the time is the scattered ~100-byte runs of `w` (one per incident segment,
// ~3 TB/s of real traffic).  A flat variant (a node's contributing cycles as ONE contiguous range of two static streams, column + cycle
// index, every lane of every load busy, no segment records) was built and measured: 250 vs 228 us at C4, 29.7 vs 27.0 at C2, 404 vs 392 at
// C5 -- its 4 extra bytes per entry cost more than the idle lanes of the 16-lanes-per-segment form; removed again.  Two adjacent cycles per lane
// (16-byte loads, what gained 4-5 % in the band sweep): 309 vs 238 us -- half as many independent requests in flight per wave; removed too.
constexpr int COLSUM_U = 8;
// The LAST workgroup of the launch does no column at all: it runs the bookkeeping of the previous sweep (traces,
// stop rule) that used to be a separate one-wave launch per iteration.  If it sets the stop flag while the
// node workgroups of this launch are running, they finish a T that nobody reads: the sweep that follows returns at once.
// The column of every contributing cycle comes from `midx`: a static stream of 16-bit column indices in exactly the order this
// kernel consumes them (node-major, then incident segment, then contributing cycle; `moff` = start of a CSR slot's run), read
// sequentially -- instead of the 4-byte packed words of the cycles, which sit in scattered 50-byte runs next to the weights
// (round 2: -25 % of this pass's sectors).
// Walks the segments [0, nrun) of one node's run (records in LDS: sb = first contributing cycle, sc = their number, sm = start in midx)
// in groups of SPI = 64 / CL consecutive segments, first group g_first, then every g_step-th, adding each contributing cycle's weight to
// column midx[..] of `cols`.  COLSUM_U groups are in flight per wave.
//
// The columns are 64-bit FIXED-POINT sums (round 4): a weight lies in [0, 1], a column adds at most one cycle of every incident segment, so
// round(w * 2^fx_bits) with fx_bits = 62 - ceil(log2(max degree + 1)) never overflows and costs <= 2^-(fx_bits+1) per term (2.2e-16 at C4,
// below the rounding of a double sum of the same terms).  Integer adds commute: the sum does not depend on the order in which lanes, waves or
// the LDS unit apply them, so the pass is bitwise reproducible BY CONSTRUCTION, and ONE copy of the columns per workgroup serves all four
// waves (a quarter of the accumulator LDS: 3 -> 7 workgroups per CU at C4).  History: rounds 1-3 kept per-wave copies of doubles and relied on
// the LDS unit resolving same-address lanes of one ds_add_f64 in a fixed order (observed, not specified); the order-explicit form of that
// (one segment of an instruction after the other) measured +10 % on this kernel (profiles/r04_ab_colsum_ordered_and_descriptors.txt: C4 230 ->
// 253 us, C2 27.0 -> 29.5); the fixed-point form had measured -5 % in round 3 (profiles/r03_colsum_bound.txt) and was shelved then.
template <int CL>
__device__ __forceinline__ void colsum_walk(unsigned long long* cols, const int* sb, const int* sc, const uint32_t* sm, int nrun, int g_first, int g_step,
                                            const uint16_t* midx, const double* w, int lane, double fx_scale) {
    // Inside a segment the cycles are ordered [(ik;j) only | both mirrors | (jk;i) only |
    // none], so either endpoint reads one run: only the `nact` cycles that contribute to its
    // columns (~n_sample/codeg of them; the smaller endpoint the first two classes, the larger
    // the middle two).  A wave instruction serves 4 segments x 16 lanes; segments
    // with more than 16 contributing cycles take further passes.  Every load of a batch is
    // issued before any result is touched (a use between loads would make the compiler wait
    // for each one).
    // CL lanes per segment, i.e. 2 CL slots per segment and round.  16 is right when a segment has 12-25 contributing cycles per endpoint
    // (C2, C3, C4); with ~9 (C5: 30 sampled cycles, 30 % of them with a sampled mirror) half of a 16-lane group's loads and adds are
    // idle: 8 lanes and 8 segments per instruction there -- C5 389.5 -> 370 us; at C4 / C3 / C2 the narrower groups cost +2.6 / +2.7 / +15 %
    // (second rounds), so the host picks by the average run length (setup_node).
    constexpr int SPI = 64 / CL;          // segments per wave instruction
    const int sub = lane / CL, l16 = lane % CL;
    for (int g0 = g_first; SPI * g0 < nrun; g0 += g_step * COLSUM_U) {
        // pieces 0 and 1 (contributing cycles 0..31 of each segment) are loaded together;
        // segments with more take further rounds
        for (int round = 0; round < MAX_SEG_CYCLES / (2 * CL); ++round) {
            uint32_t pv[2 * COLSUM_U]; double wvv[2 * COLSUM_U];
            bool more = false;
#pragma unroll
            for (int u = 0; u < COLSUM_U; ++u) {
                const int tt = SPI * (g0 + g_step * u) + sub;
                pv[2 * u] = 0xFFFFu; pv[2 * u + 1] = 0xFFFFu; wvv[2 * u] = 0.0; wvv[2 * u + 1] = 0.0;
                if (tt < nrun) {
                    const int nact = sc[tt] & 0x1FF;
                    more |= nact > 2 * CL * (round + 1);
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2) {
                        const int q = l16 + CL * (2 * round + h2);
                        if (q < nact) {
                            const int64_t c = (int64_t)sb[tt] + q;          // (as buffer loads, like the band sweep's: no change, 239.1 vs 239.0 us at C4)
                            pv[2 * u + h2] = midx[(size_t)sm[tt] + q];
                            wvv[2 * u + h2] = w[c];
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 2 * COLSUM_U; ++u)
                if (pv[u] != 0xFFFFu) atomicAdd(&cols[pv[u]], (unsigned long long)__double2ll_rn(wvv[u] * fx_scale));      // ds_add_u64
            if (!__any(more)) break;
        }
    }
}

// LDS: `copies` x stride_cols 64-bit columns (1: the workgroup's shared copy; 4: one per wave, when the launch has short-run nodes), then 3 ints per incident edge
template <int CL>
__global__ __launch_bounds__(256) void k_colsum_node(const int32_t* rowptr, const int2* adj_seg, const uint32_t* moff, const uint16_t* midx, const double* w,
                                                     double* Tfull, int n, int stride_cols, const DevState* st, const int32_t* xpos, FinArgs fin, int32_t* tail_ticket, const int32_t* node_order,
                                                     const int2* node_run, int n_long, int copies, double fx_scale) {
    if (blockIdx.x == gridDim.x - 1) {
        if (fin.st) finalize_block(fin);
        if (threadIdx.x < 8 && tail_ticket) tail_ticket[threadIdx.x] = 0;      // the sweep launches that follow (one per exchange part) hand out their tail pieces from 0
        return;
    }
    if (st->stop) return;
    extern __shared__ unsigned long long acc[];
    int* seg_base = (int*)(acc + copies * stride_cols);
    int* seg_cf = seg_base + stride_cols;             // slot_record: {first contributing cycle, their number (| flag)}
    uint32_t* seg_mo = (uint32_t*)(seg_cf + stride_cols);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // node_order lists the nodes to visit (the dispatcher hands workgroups out in index order: see setup_node for the order), first the
    // n_long nodes that get a workgroup each, then the short-run nodes of a sharded run, four per workgroup
    if ((int)blockIdx.x < n_long) {
        const int vi = blockIdx.x;
        const int v = node_order ? node_order[vi] : vi;
        const int r0 = rowptr[v], deg = rowptr[v + 1] - r0;
        if (deg == 0) return;
        // Sharded runs: the segments of row v this rank owns -- those whose smaller endpoint lies in its node range -- are ONE contiguous run
        // [run.x, run.y) of the row's CSR slots (neighbours ascending); only that run is loaded and walked.  One rank: the whole row.
        const int2 run = node_run ? node_run[v] : int2{0, deg};
        const int ra = r0 + run.x, nrun = run.y - run.x;
        for (int t = threadIdx.x; t < deg; t += 256) acc[t] = 0ull;
        for (int t = threadIdx.x; t < nrun; t += 256) {    // CSR-aligned segment records: one coalesced load
            const int2 rec = adj_seg[ra + t];
            seg_base[t] = rec.x; seg_cf[t] = rec.y; seg_mo[t] = moff[ra + t];
        }
        __syncthreads();
        // groups of segments are dealt to the four waves round-robin; all add into the one shared copy
        colsum_walk<CL>(acc, seg_base, seg_cf, seg_mo, nrun, wv, 4, midx, w, lane, fx_scale);
        __syncthreads();
        for (int t = threadIdx.x; t < deg; t += 256)
            Tfull[xpos ? xpos[r0 + t] : r0 + t] = __longlong_as_double((long long)acc[t]);   // the fixed-point bits (fx_to_double); xpos: owner-sorted exchange layout
        return;
    }
    // Short runs (sharded ranks: most rows hold only a few dozen of a rank's segments -- at C4 over 8 GPUs rank 0 visits 4670 rows with ~66 of
    // its segments each): one WAVE per node, its copy of the columns wave-private, no barrier; four nodes per workgroup.  Measured per rank
    // before (a workgroup per node): 50-79 us by rank for ~29 us worth of entries (profiles/r04_shard_w8_c4_default.json).
    const int vi = n_long + ((int)blockIdx.x - n_long) * 4 + wv;
    if (vi >= n) return;
    const int v = node_order[vi];
    const int r0 = rowptr[v], deg = rowptr[v + 1] - r0;
    const int2 run = node_run[v];
    const int ra = r0 + run.x, nrun = min(run.y - run.x, COLSUM_SHORT);
    unsigned long long* mine = acc + wv * stride_cols;
    int* sb = seg_base + wv * COLSUM_SHORT; int* sc = seg_cf + wv * COLSUM_SHORT; uint32_t* sm = seg_mo + wv * COLSUM_SHORT;
    for (int t = lane; t < deg; t += 64) mine[t] = 0ull;
    for (int t = lane; t < nrun; t += 64) {
        const int2 rec = adj_seg[ra + t];
        sb[t] = rec.x; sc[t] = rec.y; sm[t] = moff[ra + t];
    }
    __builtin_amdgcn_wave_barrier();                  // one wave: its LDS operations execute in program order
    colsum_walk<CL>(mine, sb, sc, sm, nrun, 0, 1, midx, w, lane, fx_scale);
    __builtin_amdgcn_wave_barrier();
    for (int t = lane; t < deg; t += 64) Tfull[xpos ? xpos[r0 + t] : r0 + t] = __longlong_as_double((long long)mine[t]);
}

__global__ __launch_bounds__(256) void k_init_node(const int32_t* cum, const EdgeInfo* einfo, const double* S0,
                                                   double* w, double* S_a, double* S_b, int m_pos, double* s_slice, const int2* xt) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t l = wid; l < m_pos; l += nw) {
        const int base = cum[l], cnt = cum[l + 1] - base;
        const double w0 = 1.0 / (double)cnt;
        double s = 0.0;
        for (int t = lane; t < cnt; t += 64) { w[(int64_t)base + t] = w0; s += w0 * S0[(int64_t)base + t]; }
        s = group_sum<64>(s);
        if (lane == 0) {
            const EdgeInfo ei = einfo[l];
            S_a[ei.slot_a] = s; S_a[ei.slot_b] = s; S_b[ei.slot_a] = s; S_b[ei.slot_b] = s;
            if (s_slice) s_slice[xt[l].x] = s;
        }
    }
}

__global__ __launch_bounds__(256) void k_objective_node(const int32_t* cum, const EdgeInfo* einfo, const uint32_t* pk,
                                                        const double* w, const double* S, int m_pos, double* partials,
                                                        const DevState* st) {
    if (st->stop) return;
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * 256) >> 6;
    double acc = 0.0;
    for (int64_t l = wid; l < m_pos; l += nw) {
        const int base = cum[l], cnt = cum[l + 1] - base;
        const EdgeInfo ei = einfo[l];
        for (int t = lane; t < cnt; t += 64) {
            const uint32_t p = pk[(int64_t)base + t];
            acc += w[(int64_t)base + t] * (S[ei.rb_j + (int)((p >> 16) & 0x7FFFu)] + S[ei.rb_i + (int)(p & 0x7FFFu)]);
        }
    }
    block_partials(acc, 0.0, partials, blockIdx.x);
}

// S_vec in the caller's edge order from the CSR-aligned copy
__global__ void k_extract_S(const double* Sfull, const int32_t* eslot, double* S_vec, int64_t m) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x)
        S_vec[e] = Sfull[eslot[e]];
}
// per-cycle vector between natural order and device order (dir 0: natural -> device, 1: device -> natural)
__global__ __launch_bounds__(256) void k_reorder_cycles(const int32_t* cum, const int32_t* src_start, const uint8_t* seg_perm,
                                                        const double* in, double* out, int m_pos, int dir) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t l = wid; l < m_pos; l += nw) {
        const int base = cum[l], cnt = cum[l + 1] - base, src = src_start[l];
        for (int t = lane; t < cnt; t += 64) {
            const int o = seg_perm[(int64_t)base + t];          // natural offset of the cycle stored at device slot t
            if (dir == 0) out[(int64_t)base + t] = in[(int64_t)src + o];
            else out[(int64_t)src + o] = in[(int64_t)base + t];
        }
    }
}

// ---- multi-GPU exchange helpers (node variant) --------------------------------
// A rank's all-gather slice = [S of the edges it owns, padded to the largest shard | SHARD_PARTS pairs of workgroup
// partials (objective, sum |dS|)].  The sweep kernels write both straight into the slice; after the all-gather
// k_unpack_S scatters S of every edge into both of its CSR slots, and its extra last workgroup adds all ranks'
// partials in rank order (identical sums, hence identical stop decisions, on every rank) and runs the stop rule.
__global__ __launch_bounds__(256) void k_unpack_S(const int32_t* spos, int64_t nslots, const double* sall, double* S_a, double* S_b, FinArgs fin) {
    if (blockIdx.x == 0) {                      // the bookkeeping workgroup: dispatched first, runs under the copy
        if (fin.t > 0) finalize_block(fin);
        return;
    }
    // once the stop rule has fired the slices hold the discarded sweep: the double buffers must keep the final iterate
    if (fin.st->stop || !S_a) return;
    // every CSR slot from its place in the gathered slices: coalesced writes; reads contiguous for the larger-neighbour half of a row
    // (four independent position -> value chains in flight per thread.  Round 4, rocprofv3 over the eight emulated ranks of C4 on one card,
    //  profiles/r04_shard_w8_c4_rocprof.txt: 73 us on average but 35 us at best -- the eight ranks' tables (8 x 80 MB) evict each other from the
    //  256 MB Infinity Cache between a rank's turns, which a rank on its own GPU does not suffer.  A tile-ordered form -- slots visited
    //  (tile of source nodes)-major so that the gathered values stay in the L2 -- measured 81 us on average, 53 at best: not adopted.)
    const int64_t stride = (int64_t)(gridDim.x - 1) * 256;
    for (int64_t t = (int64_t)(blockIdx.x - 1) * 256 + threadIdx.x; t < nslots; t += 4 * stride) {
        int32_t q[4]; double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = spos[min(t + u * stride, nslots - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = sall[q[u]];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (t + u * stride < nslots) {
                S_a[t + u * stride] = v[u];
                if (S_b) S_b[t + u * stride] = v[u];
            }
    }
}

// ===========================================================================
// shared small kernels
// ===========================================================================
__global__ void k_fill(double* p, int64_t n, double v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

namespace {

void free_all(desc_pgd* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();                              // once for all blocks and both streams (dev_free would wait per block)
    for (void* q : h->allocs) dev_free_idle(q);
    for (hipEvent_t e : {h->ev_col, h->ev_rs, h->ev_sw, h->ev_ag}) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->ev_rsx) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->ev_ext) if (e) (void)hipEventDestroy(e);
    stream_release(h->comm_stream);
    if (!h->borrowed_stream) stream_release(h->stream);
    delete h;
}

// the bookkeeping of the last enqueued sweep, if it is still waiting for a column-sum launch to ride on
void flush_finalize(desc_pgd* h) {
    if (!h->pending_fin) return;
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, h->stream, fin_args(h, h->d_partials, h->pending_parts, h->pending_fin, 0));
    h->pending_fin = 0;
}

// column copies in the LDS of k_colsum_node: one shared by the workgroup; four (one per wave) when the launch has short-run nodes, a wave each
int colsum_copies(const desc_pgd* h) { return h->colsum_long < h->colsum_nodes ? 4 : 1; }
size_t colsum_lds(const desc_pgd* h) { return (size_t)h->colsum_stride * (colsum_copies(h) * sizeof(unsigned long long) + 3 * sizeof(int)); }

// enqueue sweep number t (1-based) and its finalize; ev0/ev1 bracket the kernels of the sweep proper
int enqueue_sweep(desc_pgd* h, int t, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr) {
    const int rd = (t - 1) & 1, wr = t & 1;
    bool adam = false;
    const StepArgs st = make_step(h, &adam, rd, wr);
    int rc;
    if (ev0) (void)hipEventRecord(ev0, h->stream);
    if (h->variant == VARIANT_NODE) {
        const FinArgs fin = fin_args(h, h->d_partials, h->pending_parts, h->pending_fin, 0);      // the previous sweep's bookkeeping rides on this launch
        launch_colsum(h, h->stream, h->d_w[rd], h->d_T, nullptr, fin);
        h->pending_fin = 0;
        NodeSweepArgs a = node_sweep_args(h, rd, wr);
        a.Tfull = h->d_T; a.partials = h->d_partials; a.st = st; a.t_bytes = a.csr_bytes;       // xt, s_slice: NULL, slice_bytes: 0
        if ((rc = launch_sweep_node_layout(h, a, adam))) return rc;
    } else {
        SweepArgs a{};
        a.cum = h->d_cum; a.pos_edge = h->d_pos_edge; a.e_jk = h->d_ejk; a.e_ki = h->d_eki; a.ikj = h->d_ikj; a.jki = h->d_jki;
        a.S0 = h->d_S0; a.w_old = h->d_w[rd]; a.w_new = h->d_w[wr]; a.S_old = h->d_S[rd]; a.S_new = h->d_S[wr];
        a.nv_tab = h->d_nv; a.partials = h->d_partials; a.state = h->d_state; a.st = st;
        a.m_pos = (int32_t)h->m_pos;
        if ((rc = launch_gather(h, a, adam))) return rc;
    }
    if (ev1) (void)hipEventRecord(ev1, h->stream);
    h->pending_fin = t; h->pending_parts = sweep_parts(h, adam, true);
    if (h->variant != VARIANT_NODE) flush_finalize(h);         // no column-sum launch to ride on
    DESC_HIP(hipGetLastError());
    return DESC_OK;
}

// the next n sweeps.  (hipGraph replays of 10 captured iterations were built in round 3 and measured no gain -- C1 16.5 vs 16.6 us per
// iteration, C2 0.150 vs 0.152 ms, profiles/r03_graph_ab.txt: each kernel is a chain of dependent memory round trips, the launches were not
// what an iteration waits for -- and removed in round 4.)
int enqueue_iterations(desc_pgd* h, int n) {
    for (; n > 0; --n) { const int rc = enqueue_sweep(h, ++h->t_done); if (rc) return rc; }
    return DESC_OK;
}

// per-cycle host vector <-> device (handles the node layout's segment permutation)
int cycles_to_device(desc_pgd* h, const double* host, double* dev) {
    if (h->m_cycle == 0) return DESC_OK;
    if (h->variant != VARIANT_NODE) { DESC_HIP(hipMemcpyAsync(dev, host, sizeof(double) * h->m_cycle, hipMemcpyHostToDevice, h->stream)); return DESC_OK; }
    DESC_HIP(hipMemcpyAsync(h->d_scratch, host, sizeof(double) * h->m_cycle, hipMemcpyHostToDevice, h->stream));
    int g = (int)std::min<int64_t>(4096, (h->m_pos + 3) / 4);
    hipLaunchKernelGGL(k_reorder_cycles, dim3(g), dim3(256), 0, h->stream, h->d_cum + h->seg_lo, h->d_src_start + h->seg_lo, h->d_seg_perm, h->d_scratch, dev, (int)(h->seg_hi - h->seg_lo), 0);
    return DESC_OK;
}
int cycles_to_host(desc_pgd* h, const double* dev, double* host) {
    if (h->m_cycle == 0) return DESC_OK;
    if (h->variant != VARIANT_NODE) { DESC_HIP(hipMemcpy(host, dev, sizeof(double) * h->m_cycle, hipMemcpyDeviceToHost)); return DESC_OK; }
    int g = (int)std::min<int64_t>(4096, (h->m_pos + 3) / 4);
    hipLaunchKernelGGL(k_reorder_cycles, dim3(g), dim3(256), 0, h->stream, h->d_cum + h->seg_lo, h->d_src_start + h->seg_lo, h->d_seg_perm, dev, h->d_scratch, (int)(h->seg_hi - h->seg_lo), 1);
    DESC_HIP(hipStreamSynchronize(h->stream));
    DESC_HIP(hipMemcpy(host, h->d_scratch, sizeof(double) * h->m_cycle, hipMemcpyDeviceToHost));      // synchronous: nothing stays pending into caller memory
    return DESC_OK;
}
int ensure_scratch(desc_pgd* h) {
    if (h->d_scratch || h->variant != VARIANT_NODE) return DESC_OK;
    return dalloc(h, &h->d_scratch, h->m_cycle);
}

// HybridGradient keeps m_t / v_t between calls (handle object): after desc_pgd_reset, the caller's moments of a run that
// continues (t0 > 0) go to the parity sweep 1 reads
int upload_adam_state(desc_pgd* h, const desc_params* p, const desc_result* r) {
    if (!(p->step_kind == DESC_STEP_HYBRID && p->hybrid_strategy == 0 && p->t0 > 0 && r->adam_m && r->adam_v && h->m_cycle > 0)) return DESC_OK;
    int rc = ensure_scratch(h); if (rc) return rc;
    rc = cycles_to_device(h, r->adam_m, h->d_adam_m[0]); if (rc) return rc;
    DESC_HIP(hipStreamSynchronize(h->stream));
    rc = cycles_to_device(h, r->adam_v, h->d_adam_v[0]); if (rc) return rc;
    DESC_HIP(hipStreamSynchronize(h->stream));
    return DESC_OK;
}

// what desc_pgd_iterate and desc_pgd_iterate_timed refuse; then the handle's device is current
int iterate_begin(const desc_pgd* h, int32_t n_iters) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    if (!h->armed) return fail(DESC_ERR_STATE, "desc_pgd_reset must be called first");
    if (h->ext_phase) return fail(DESC_ERR_STATE, "the handle runs a caller-supplied step rule (desc_pgd_ext_begin): iterate with desc_pgd_ext_grad / desc_pgd_ext_apply");
    if (n_iters < 0 || h->t_done + n_iters > h->iters_cap) return fail(DESC_ERR_INVALID, "iterating past params.iters = %d", h->p.iters);
    return set_device(h);
}

int create_impl(const desc_problem* prob, const double* shared_rij, const desc_structure* s, int32_t device, int32_t rank, int32_t world,
                desc_pgd** out) {
    if (!out) return fail(DESC_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!prob || !s) return fail(DESC_ERR_INVALID, "NULL argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(DESC_ERR_INVALID, "rank %d / world %d", rank, world);
    if (prob->m != s->m) return fail(DESC_ERR_INVALID, "structure was built for m = %lld, problem has m = %lld", (long long)s->m, (long long)prob->m);
    if (prob->m > 0 && !prob->rij && !shared_rij) return fail(DESC_ERR_INVALID, "rij is NULL");
    if (prob->n < s->n) return fail(DESC_ERR_INVALID, "problem n smaller than structure n");
    int ndev = desc_device_count();
    if (ndev < 0) return ndev;
    if (ndev == 0) return fail(DESC_ERR_HIP, "no HIP device visible: the DESC_PGD hot path has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(DESC_ERR_INVALID, "device %d out of range (0..%d)", device, ndev - 1);

    desc_pgd* h = new (std::nothrow) desc_pgd();
    if (!h) return fail(DESC_ERR_INVALID, "out of host memory");
    h->device = device; h->rank = rank; h->world = world;
    h->n = prob->n; h->m = s->m; h->m_pos = s->m_pos; h->m_cycle = s->m_cycle; h->max_cnt = s->max_cnt; h->n_sample = s->n_sample;
    if (s->max_deg > 0) h->max_deg = s->max_deg;          // device-built structures carry it
    else {
        hvec<int32_t> deg((size_t)h->n, 0);
        for (int64_t e = 0; e < h->m; ++e) { deg[prob->ind_i[e]]++; deg[prob->ind_j[e]]++; }
        for (int32_t d : deg) h->max_deg = std::max(h->max_deg, d);
    }
    int rc = DESC_OK;
    hipError_t he = hipSetDevice(device);
    if (he == hipSuccess) he = stream_acquire(&h->stream);
    if (he != hipSuccess) { rc = fail(DESC_ERR_HIP, "device %d: %s", device, hipGetErrorString(he)); free_all(h); return rc; }

    // variant: NODE unless the packed per-cycle word or the LDS column copies do not fit
    const int forced = env_int("DESC_DEBUG_VARIANT", 0);
    const bool node_ok = h->max_deg < 32768 && (size_t)(h->max_deg + 2) * 44 <= 150 * 1024 && h->max_cnt <= MAX_SEG_CYCLES && h->m_pos > 0;
    h->variant = (forced == VARIANT_GATHER || !node_ok) ? VARIANT_GATHER : VARIANT_NODE;
    if (world > 1 && h->variant != VARIANT_NODE) {
        rc = fail(DESC_ERR_INVALID, "multi-GPU sharding needs the node layout (max degree < 2^15, segments <= 64 cycles)");
        free_all(h); return rc;
    }

    const int64_t mp = h->m_pos, mc = h->m_cycle;
    auto A = [&](int r) { if (!rc) rc = r; };
    A(dalloc(h, &h->d_cum, mp + 1));
    if (h->variant != VARIANT_NODE) { A(dalloc(h, &h->d_S0, mc)); A(dalloc(h, &h->d_w[0], mc)); A(dalloc(h, &h->d_w[1], mc)); }
    A(dalloc(h, &h->d_nv, (size_t)h->max_cnt + 1));
    A(dalloc(h, &h->d_state, 1));
    if (!rc) {
        hvec<double> nv((size_t)h->max_cnt + 1, 0.0);
        for (int c = 1; c <= h->max_cnt; ++c) nv[c] = 1.0 / std::pow((double)c, 0.5);   // ones/(nsample^0.5), DESC_PGD.m:199
        rc = upload(h, h->d_nv, nv.data(), nv.size());
        if (!rc) { hipError_t e = hipStreamSynchronize(h->stream); if (e != hipSuccess) rc = fail(DESC_ERR_HIP, "upload: %s", hipGetErrorString(e)); }
    }
    if (!rc) rc = (h->variant == VARIANT_NODE) ? setup_node(h, prob, s, shared_rij) : setup_gather(h, prob, s, shared_rij);
    if (!rc) rc = dalloc(h, &h->d_partials, 4 * parts_cap(h));   // sweep partials, then the objective kernel's
    if (rc) { free_all(h); return rc; }
    *out = h;
    return DESC_OK;
}

}  // namespace

StepArgs make_step(desc_pgd* h, bool* adam, int rd, int wr) {
    const desc_params& p = h->p;
    StepArgs s{};
    s.adam_m = h->d_adam_m[rd]; s.adam_v = h->d_adam_v[rd]; s.adam_m_out = h->d_adam_m[wr]; s.adam_v_out = h->d_adam_v[wr];
    // one GetStep call per iteration (DESC_PGD.m:207): the plugin counter advances first
    *adam = plugin_step(p, ++h->t_plugin, s);
    return s;
}

// second half of d_partials: the objective kernel of a download writes there, so the partials of the last sweep stay intact and
// book-keeping that sweep again (a replayed column-sum launch after a flush or a download) rewrites the same numbers
size_t parts_cap(const desc_pgd* h) { return (size_t)std::max(std::max(std::max(h->grid, h->obj_grid), h->band_grid + h->band_ntail), h->small_grid); }
double* obj_partials(const desc_pgd* h) { return h->d_partials + 2 * parts_cap(h); }
FinArgs fin_args(const desc_pgd* h, const double* partials, int nparts, int t, int last_only) {
    return FinArgs{partials, h->d_state, h->d_obj, h->d_avg, h->m, h->p.stop_tol, nparts, t, h->p.patience, last_only, 0, 1};
}

// once per handle (setup_node, with colsum_stride and the node list known): the fixed-point position of the column sums, and room for the longest
// row's columns in the dynamic LDS of both instances
int prepare_colsum(desc_pgd* h) {
    int bits = 0;
    while ((1 << bits) < h->max_deg + 1) ++bits;
    h->colsum_fx_bits = 62 - bits;
    const size_t lds = colsum_lds(h);
    if (lds > 64 * 1024)
    {
        DESC_HIP(hipFuncSetAttribute((const void*)k_colsum_node<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        DESC_HIP(hipFuncSetAttribute((const void*)k_colsum_node<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    return DESC_OK;
}

// the column-sum pass over the weights `w` -> T (through xpos: the exchange layout of a sharded run); `fin`: the bookkeeping that rides on it
void launch_colsum(desc_pgd* h, hipStream_t st, const double* w, double* T, const int32_t* xpos, const FinArgs& fin) {
    const dim3 grid(h->colsum_grid + 1), block(256);
    const size_t lds = colsum_lds(h);
    const int copies = colsum_copies(h);
    const double fx_scale = std::ldexp(1.0, h->colsum_fx_bits);
    if (h->colsum_cl == 8)
        hipLaunchKernelGGL(k_colsum_node<8>, grid, block, lds, st, h->d_rowptr, h->d_adj_seg, h->d_moff, h->d_midx, w, T, h->colsum_nodes, h->colsum_stride, h->d_state,
                           xpos, fin, h->d_ticket, h->d_node_order, h->d_node_run, h->colsum_long, copies, fx_scale);
    else
        hipLaunchKernelGGL(k_colsum_node<16>, grid, block, lds, st, h->d_rowptr, h->d_adj_seg, h->d_moff, h->d_midx, w, T, h->colsum_nodes, h->colsum_stride, h->d_state,
                           xpos, fin, h->d_ticket, h->d_node_order, h->d_node_run, h->colsum_long, copies, fx_scale);
}

// what every sweep on the node layout is given, one rank or sharded; the caller adds Tfull, xt, s_slice, partials, t_bytes, slice_bytes and the step
NodeSweepArgs node_sweep_args(const desc_pgd* h, int rd, int wr) {
    NodeSweepArgs a{};
    a.cum = h->d_cum; a.einfo = h->d_einfo; a.pk = h->d_pk; a.S0 = h->d_S0; a.w_old = h->d_w[rd]; a.w_new = h->d_w[wr];
    a.S_old = h->d_S[rd]; a.S_new = h->d_S[wr]; a.nv_tab = h->d_nv;
    a.state = h->d_state; a.chunk_desc = h->d_chunk_desc + h->ch_lo; a.nchunks = h->nchunks; a.max_cnt = h->max_cnt;
    a.csr_bytes = (uint32_t)(16 * h->m); a.seg_count = (uint32_t)h->m_pos; a.fx_inv = std::ldexp(1.0, -h->colsum_fx_bits);
    return a;
}

// The objective (DESC_PGD.m:233) of the iterate in the buffers of parity `par`, as `grid` pairs of workgroup partials at `partials`: over this rank's
// segments on the node layout, over all cycles on the gather layout.  After the last sweep (desc_pgd_download), for the final exchange of a sharded
// run (pgd_shard.hip) and after every applied step of a caller-supplied rule (pgd_ext.hip).
void launch_objective(desc_pgd* h, hipStream_t st, int par, int grid, double* partials) {
    if (h->variant == VARIANT_NODE)
        hipLaunchKernelGGL(k_objective_node, dim3(grid), dim3(256), 0, st, h->d_cum + h->seg_lo, h->d_einfo + h->seg_lo, h->d_pk,
                           h->d_w[par], h->d_S[par], (int)(h->seg_hi - h->seg_lo), partials, h->d_state);
    else
        hipLaunchKernelGGL(k_objective, dim3(grid), dim3(256), 0, st, h->d_w[par], h->d_S[par], h->d_ejk,
                           h->d_eki, h->m_cycle, partials, h->d_state);
}

// k_unpack_S behind the all-gather of a sharded run (pgd_shard.hip: shard_enqueue_unpack): `g` copy workgroups behind the bookkeeping workgroup
void launch_unpack(desc_pgd* h, hipStream_t st, int g, double* S_a, double* S_b, const FinArgs& f) {
    hipLaunchKernelGGL(k_unpack_S, dim3(g + 1), dim3(256), 0, st, h->d_spos, (int64_t)2 * h->m, h->x_sall, S_a, S_b, f);
}

int pgd_create_with_rij(const desc_problem* prob, const double* d_rij, const desc_structure* s, int32_t device, desc_pgd** out) {
    return create_impl(prob, d_rij, s, device, 0, 1, out);
}

}  // namespace desc

using namespace desc;

extern "C" {

int desc_pgd_create(const desc_problem* prob, const desc_structure* s, int32_t device, desc_pgd** out) {
    return desc_pgd_create_shard(prob, s, device, 0, 1, out);
}

int desc_pgd_create_shard(const desc_problem* prob, const desc_structure* s, int32_t device, int32_t rank, int32_t world,
                          desc_pgd** out) {
    return no_throw("desc_pgd_create_shard", [&]() -> int {
    return create_impl(prob, nullptr, s, device, rank, world, out);
    });
}
// the same with the problem already resident in HBM (desc_problem_upload): nothing but O(m_pos) plan tables is uploaded
int desc_pgd_create_dev(const desc_device_problem* dp, const desc_structure* s, int32_t rank, int32_t world, desc_pgd** out) {
    return no_throw("desc_pgd_create_dev", [&]() -> int {
    if (!dp) return fail(DESC_ERR_INVALID, "NULL argument");
    const desc_problem hv = host_view(dp);
    return create_impl(&hv, dp->d_rij, s, dp->device, rank, world, out);
    });
}

void desc_pgd_destroy(desc_pgd* h) { free_all(h); }

int desc_pgd_sizes(const desc_pgd* h, int64_t* m, int64_t* m_pos, int64_t* m_cycle, int32_t* max_cnt) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    if (m) *m = h->m;
    if (m_pos) *m_pos = h->m_pos;
    if (m_cycle) *m_cycle = h->m_cycle;
    if (max_cnt) *max_cnt = h->max_cnt;
    return DESC_OK;
}

const char* desc_pgd_kernel_name(const desc_pgd* h) { return h ? h->kname.c_str() : ""; }

int desc_pgd_get_s0(desc_pgd* h, double* s0) {
    if (!h || !s0) return fail(DESC_ERR_INVALID, "NULL argument");
    int rc = set_device(h); if (rc) return rc;
    if ((rc = ensure_scratch(h))) return rc;
    return cycles_to_host(h, h->d_S0, s0);
}

int desc_pgd_reset(desc_pgd* h, const desc_params* p) {
    if (!h || !p) return fail(DESC_ERR_INVALID, "NULL argument");
    if (p->iters < 0) return fail(DESC_ERR_INVALID, "iters < 0");
    if (p->step_kind == DESC_STEP_EXTERNAL)
        return fail(DESC_ERR_INVALID, "step_kind DESC_STEP_EXTERNAL: the caller supplies the step, through desc_pgd_ext_begin / desc_pgd_ext_grad / desc_pgd_ext_apply");
    if (p->step_kind < 0 || p->step_kind > 2) return fail(DESC_ERR_INVALID, "unknown step_kind %d", p->step_kind);
    if ((p->step_kind == DESC_STEP_PIECEWISE || (p->step_kind == DESC_STEP_HYBRID && p->hybrid_strategy == 1)) && !(p->decay_interval > 0))
        return fail(DESC_ERR_INVALID, "decay_interval must be > 0");
    int rc = set_device(h); if (rc) return rc;
    h->p = *p;
    if (h->p.patience <= 0) h->p.patience = 30;
    {   // diagnostics only: never set in production runs
        const int gr = env_int("DESC_DEBUG_GRID", 0);
        if (gr >= 8 && gr / 8 * 8 != h->grid) {
            dfree(h, h->d_partials); h->d_partials = nullptr;
            h->grid = gr / 8 * 8;
            rc = dalloc(h, &h->d_partials, 4 * parts_cap(h)); if (rc) return rc;
        }
    }
    h->t_done = 0; h->t_plugin = p->t0; h->ms_pgd = 0; h->objective_done = false; h->final_obj_T = -1; h->pending_fin = 0;
    h->ext_phase = 0;

    const int cap = std::max(1, p->iters);
    h->iters_cap = cap;
    if (cap > h->trace_cap) {
        dfree(h, h->d_obj); dfree(h, h->d_avg);
        h->d_obj = h->d_avg = nullptr; h->trace_cap = 0;
        rc = dalloc(h, &h->d_obj, cap); if (rc) return rc;
        rc = dalloc(h, &h->d_avg, cap); if (rc) return rc;
        h->trace_cap = cap;
    }
    if (p->step_kind == DESC_STEP_HYBRID && p->hybrid_strategy == 0 && !h->d_adam_m[0])
        for (int q = 0; q < 2; ++q) {
            rc = dalloc(h, &h->d_adam_m[q], local_cycles(h)); if (rc) return rc;
            rc = dalloc(h, &h->d_adam_v[q], local_cycles(h)); if (rc) return rc;
        }
    DESC_HIP(hipMemsetAsync(h->d_state, 0, sizeof(DevState), h->stream));
    DESC_HIP(hipMemsetAsync(h->d_obj, 0, sizeof(double) * h->trace_cap, h->stream));
    DESC_HIP(hipMemsetAsync(h->d_avg, 0, sizeof(double) * h->trace_cap, h->stream));
    if (h->d_adam_m[0])
        for (int q = 0; q < 2; ++q) {
            DESC_HIP(hipMemsetAsync(h->d_adam_m[q], 0, sizeof(double) * std::max<int64_t>(1, local_cycles(h)), h->stream));
            DESC_HIP(hipMemsetAsync(h->d_adam_v[q], 0, sizeof(double) * std::max<int64_t>(1, local_cycles(h)), h->stream));
        }
    const int64_t slen = h->variant == VARIANT_NODE ? 2 * h->m : h->m;
    if (slen > 0) {                                                       // S_vec = ones(1,m)  (:148)
        int g = (int)std::min<int64_t>(1024, (slen + 255) / 256);
        hipLaunchKernelGGL(k_fill, dim3(g), dim3(256), 0, h->stream, h->d_S[0], slen, 1.0);
        hipLaunchKernelGGL(k_fill, dim3(g), dim3(256), 0, h->stream, h->d_S[1], slen, 1.0);
    }
    if (h->x_sall && h->slice_S > 0) {          // sharded: S of the edges this rank owns, edge order; edges without cycles keep 1 (:148)
        int g = (int)std::min<int64_t>(1024, (h->slice_S + 255) / 256);
        hipLaunchKernelGGL(k_fill, dim3(g), dim3(256), 0, h->stream, h->x_sall + (int64_t)h->rank * h->slice_len, h->slice_S, 1.0);
    }
    if (h->m_pos > 0) {
        int g = (int)std::max<int64_t>(1, std::min<int64_t>(4096, (h->m_pos + 3) / 4));
        if (h->variant == VARIANT_NODE) {
            for (int c = 0; c < h->xparts; ++c) {        // per exchange part: its segments' initial S goes behind the parts before it in the slice
                const int64_t q0 = h->xseg[c], q1 = h->xseg[c + 1];
                if (q1 > q0)
                    hipLaunchKernelGGL(k_init_node, dim3(g), dim3(256), 0, h->stream, h->d_cum + q0, h->d_einfo + q0, h->d_S0, h->d_w[0], h->d_S[0], h->d_S[1], (int)(q1 - q0),
                                       h->x_sall ? h->x_sall + (int64_t)h->rank * h->slice_len + h->xslice_off[c] : (double*)nullptr, h->d_xt + q0);
            }
        } else
            hipLaunchKernelGGL(k_init, dim3(g), dim3(256), 0, h->stream, h->d_cum, h->d_pos_edge, h->d_S0, h->d_w[0], h->d_S[0], h->d_S[1], (int)h->m_pos);
    }
    DESC_HIP(hipGetLastError());
    h->armed = true;
    return DESC_OK;
}

int desc_pgd_iterate(desc_pgd* h, int32_t n_iters) {
    int rc = iterate_begin(h, n_iters); if (rc) return rc;
    if (h->m_pos == 0) { h->t_done += n_iters; h->t_plugin += n_iters; return DESC_OK; }
    return enqueue_iterations(h, n_iters);
}

int desc_pgd_iterate_timed(desc_pgd* h, int32_t n_iters, float* ms_total, float* ms_main_kernel_avg) {
    int rc = iterate_begin(h, n_iters); if (rc) return rc;
    hipEvent_t e0, e1;
    DESC_HIP(hipEventCreate(&e0)); DESC_HIP(hipEventCreate(&e1));
    hvec<hipEvent_t> ev;
    if (ms_main_kernel_avg) { ev.resize(2 * (size_t)n_iters); for (auto& e : ev) DESC_HIP(hipEventCreate(&e)); }
    DESC_HIP(hipEventRecord(e0, h->stream));
    if (h->m_pos > 0 && !ms_main_kernel_avg) { rc = enqueue_iterations(h, n_iters); if (rc) return rc; }
    else if (h->m_pos > 0)                                   // per-iteration events: direct launches
        for (int q = 0; q < n_iters; ++q) {
            rc = enqueue_sweep(h, ++h->t_done, ev[2 * q], ev[2 * q + 1]);
            if (rc) return rc;
        }
    else { h->t_done += n_iters; h->t_plugin += n_iters; }
    DESC_HIP(hipEventRecord(e1, h->stream));
    DESC_HIP(hipStreamSynchronize(h->stream));
    float ms = 0; DESC_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (ms_total) *ms_total = ms;
    if (ms_main_kernel_avg) {
        double acc = 0; int cntk = 0;
        if (h->m_pos > 0)
            for (int q = 0; q < n_iters; ++q) { float x = 0; DESC_HIP(hipEventElapsedTime(&x, ev[2 * q], ev[2 * q + 1])); acc += x; ++cntk; }
        *ms_main_kernel_avg = cntk ? (float)(acc / cntk) : 0.f;
        for (auto& e : ev) (void)hipEventDestroy(e);
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    h->ms_pgd += ms;
    return DESC_OK;
}

int desc_pgd_sync(desc_pgd* h) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    int rc = set_device(h); if (rc) return rc;
    if ((rc = shard_unpack_pending(h))) return rc;           // fused protocol: a sync leaves every enqueued iteration complete, its unpacking included
    DESC_HIP(hipStreamSynchronize(h->stream));
    if (h->comm_stream) DESC_HIP(hipStreamSynchronize(h->comm_stream));
    DESC_HIP(hipGetLastError());
    return DESC_OK;
}

int desc_pgd_download(desc_pgd* h, desc_result* r) {
    if (!h || !r) return fail(DESC_ERR_INVALID, "NULL argument");
    if (!h->armed) return fail(DESC_ERR_STATE, "nothing to download: call desc_pgd_reset first");
    if (!r->s_vec && h->m > 0) return fail(DESC_ERR_INVALID, "result.s_vec is NULL");
    int rc = set_device(h); if (rc) return rc;
    const int T = h->t_done;
    flush_finalize(h);
    if ((rc = shard_unpack_pending(h))) return rc;           // fused protocol: S and the stop rule of the last sweep
    if (h->comm_stream) DESC_HIP(hipStreamSynchronize(h->comm_stream));
    // objective of the last sweep (DESC_PGD.m:233) and its stop test
    if (h->m_pos > 0 && T >= 1 && h->world == 1 && h->final_obj_T != T) {
        h->final_obj_T = T;
        launch_objective(h, h->stream, T & 1, h->obj_grid, obj_partials(h));
        hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, h->stream, fin_args(h, obj_partials(h), h->obj_grid, T, 1));
    }
    DevState st{};
    DESC_HIP(hipStreamSynchronize(h->stream));
    DESC_HIP(hipMemcpy(&st, h->d_state, sizeof st, hipMemcpyDeviceToHost));      // synchronous: `st` is a stack slot
    DESC_HIP(hipGetLastError());
    int iters_run = T, par = T & 1;
    if (h->m_pos > 0 && st.stop) { iters_run = st.iters_run; par = st.final_parity; }
    if (h->m_pos == 0) {
        // no cycles at all: every sweep is a no-op, objective 0, so the reference
        // breaks after `patience` misses counted from iteration 2 (DESC_PGD.m:243-246)
        if (T >= h->p.patience + 1) iters_run = h->p.patience + 1;
        par = 0;
    }
    r->iters_run = iters_run;
    r->t_end = h->p.t0 + iters_run;
    if (h->m > 0) {
        if (h->variant == VARIANT_NODE) {
            int g = (int)std::min<int64_t>(1024, (h->m + 255) / 256);
            hipLaunchKernelGGL(k_extract_S, dim3(g), dim3(256), 0, h->stream, h->d_S[par], h->d_eslot, h->d_Svec, h->m);
            DESC_HIP(hipStreamSynchronize(h->stream));
            DESC_HIP(hipMemcpy(r->s_vec, h->d_Svec, sizeof(double) * h->m, hipMemcpyDeviceToHost));
        } else {
            DESC_HIP(hipMemcpy(r->s_vec, h->d_S[par], sizeof(double) * h->m, hipMemcpyDeviceToHost));
        }
    }
    if (h->world > 1 && (r->w || r->adam_m || r->adam_v))
        return fail(DESC_ERR_INVALID, "per-cycle outputs (w, Adam state) are not gathered across ranks");
    if (r->w || (h->d_adam_m[0] && r->adam_m && r->adam_v)) { rc = ensure_scratch(h); if (rc) return rc; }
    if (r->w) { rc = cycles_to_host(h, h->d_w[par], r->w); if (rc) return rc; }
    if (r->obj_trace && iters_run > 0) {
        if (h->m_pos > 0) DESC_HIP(hipMemcpy(r->obj_trace, h->d_obj, sizeof(double) * iters_run, hipMemcpyDeviceToHost));
        else std::memset(r->obj_trace, 0, sizeof(double) * iters_run);
    }
    if (r->avg_change_trace && iters_run > 0) {
        if (h->m_pos > 0) DESC_HIP(hipMemcpy(r->avg_change_trace, h->d_avg, sizeof(double) * iters_run, hipMemcpyDeviceToHost));
        else std::memset(r->avg_change_trace, 0, sizeof(double) * iters_run);
    }
    if (h->d_adam_m[0] && r->adam_m && r->adam_v) {          // the state after exactly iters_run GetStep calls
        rc = cycles_to_host(h, h->d_adam_m[par], r->adam_m); if (rc) return rc;
        rc = cycles_to_host(h, h->d_adam_v[par], r->adam_v); if (rc) return rc;
    }
    r->ms_upload = h->ms_upload; r->ms_cycle_d = h->ms_cycle_d; r->ms_pgd = h->ms_pgd;
    return DESC_OK;
}

// params.make_plots = true (DESC_PGD.m:235-239) as a composition of device rows: one sweep, one S_vec download and one GCW
// eigen-solve per iteration.  The alignment against R_orig (:238, GlobalSOdCorrectRight) stays with the caller.
int desc_pgd_run_traced(desc_pgd* h, const desc_device_problem* dp, const desc_params* p, const double* err_vec, double gcw_tol,
                        int32_t gcw_max_iters, double* svec_errors, double* R_est_all, desc_result* r) {
    return no_throw("desc_pgd_run_traced", [&]() -> int {
    if (!h || !dp || !p || !r || !err_vec || !svec_errors || !R_est_all) return fail(DESC_ERR_INVALID, "NULL argument");
    if (!r->s_vec || !r->obj_trace || !r->avg_change_trace) return fail(DESC_ERR_INVALID, "the traced run needs s_vec, obj_trace and avg_change_trace");
    if (dp->m != h->m || dp->n != h->n) return fail(DESC_ERR_INVALID, "device problem and solver handle describe different graphs");
    auto t0 = std::chrono::steady_clock::now();
    int rc = desc_pgd_reset(h, p); if (rc) return rc;
    if ((rc = upload_adam_state(h, p, r))) return rc;        // the moments stay on the device between the one-iteration pieces
    desc_result mid = *r;                                    // same buffers; w / Adam state only in the final download
    mid.w = nullptr; mid.adam_m = nullptr; mid.adam_v = nullptr;
    int done = 0;
    while (done < p->iters) {
        if ((rc = desc_pgd_iterate(h, 1))) return rc;
        ++done;
        if ((rc = desc_pgd_download(h, &mid))) return rc;    // also evaluates this iteration's objective and stop test
        if (mid.iters_run < done) break;                     // the patience rule fired at an earlier iteration (:243-246)
        double acc = 0.0;
        for (int64_t e = 0; e < h->m; ++e) acc += std::fabs(err_vec[e] - mid.s_vec[e]);
        svec_errors[done - 1] = h->m > 0 ? acc / (double)h->m : 0.0;                                     // :236
        if ((rc = desc_gcw_run_dev(dp, mid.s_vec, gcw_tol, gcw_max_iters, R_est_all + (size_t)(done - 1) * 9 * (size_t)h->n, nullptr))) return rc;   // :237
        if (p->progress) p->progress(p->progress_user, done, mid.avg_change_trace[done - 1], mid.obj_trace[done - 1]);
        else if (p->verbose) { printf("iter %d: average change in S_vec %f, objective value: %f\n", done, mid.avg_change_trace[done - 1], mid.obj_trace[done - 1]); fflush(stdout); }
    }
    rc = desc_pgd_download(h, r);
    r->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
    });
}

int desc_pgd_run(desc_pgd* h, const desc_params* p, desc_result* r) {
    return no_throw("desc_pgd_run", [&]() -> int {
    if (!h || !p || !r) return fail(DESC_ERR_INVALID, "NULL argument");
    auto t0 = std::chrono::steady_clock::now();
    int rc = desc_pgd_reset(h, p); if (rc) return rc;
    if ((rc = upload_adam_state(h, p, r))) return rc;
    // progress lines (DESC_PGD.m:241) are streamed while the loop runs: at every poll of the stop flag the traces of the
    // iterations that became final since the last poll are fetched and handed to the callback (or printed)
    const bool stream_lines = (p->progress != nullptr || p->verbose) && h->m_pos > 0;
    int chunk = p->check_every > 0 ? p->check_every : 32;
    if (stream_lines && p->check_every <= 0) chunk = 10;
    int reported = 0;
    hvec<double> lo, la;
    auto emit = [&](int it, double avg, double obj) {
        if (p->progress) p->progress(p->progress_user, it, avg, obj);
        else { printf("iter %d: average change in S_vec %f, objective value: %f\n", it, avg, obj); fflush(stdout); }
    };
    auto report_upto = [&](int upto) -> int {              // iterations reported+1 .. upto have both trace entries final
        if (upto <= reported) return DESC_OK;
        lo.resize((size_t)upto - reported); la.resize((size_t)upto - reported);
        DESC_HIP(hipMemcpy(lo.data(), h->d_obj + reported, sizeof(double) * (upto - reported), hipMemcpyDeviceToHost));
        DESC_HIP(hipMemcpy(la.data(), h->d_avg + reported, sizeof(double) * (upto - reported), hipMemcpyDeviceToHost));
        for (int it = reported + 1; it <= upto; ++it) emit(it, la[it - 1 - reported], lo[it - 1 - reported]);
        reported = upto;
        return DESC_OK;
    };
    int left = p->iters;
    while (left > 0) {
        const int nq = std::min(left, chunk);
        float ms = 0;
        rc = desc_pgd_iterate_timed(h, nq, &ms, nullptr); if (rc) return rc;
        left -= nq;
        if (left > 0 && h->m_pos > 0) {
            DevState st{};
            flush_finalize(h);
            DESC_HIP(hipStreamSynchronize(h->stream));
            DESC_HIP(hipMemcpy(&st, h->d_state, sizeof st, hipMemcpyDeviceToHost));
            // the objective of iteration t becomes known with sweep t+1: lines up to t_done - 1 (or the stop iteration) are final
            if (stream_lines && (rc = report_upto(st.stop ? st.iters_run : h->t_done - 1))) return rc;
            if (st.stop) break;
        }
    }
    rc = desc_pgd_download(h, r); if (rc) return rc;
    if (stream_lines) { if ((rc = report_upto(r->iters_run))) return rc; }
    else if ((p->verbose || p->progress) && r->obj_trace && r->avg_change_trace)      // no cycles at all: constant traces
        for (int it = 1; it <= r->iters_run; ++it) emit(it, r->avg_change_trace[it - 1], r->obj_trace[it - 1]);
    r->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return DESC_OK;
    });
}

// Diagnostics (tools/wg_clock.py): {start, end} of every workgroup of the LAST band sweep on the constant 100 MHz clock, when the handle
// was created with DESC_DEBUG_WGCLOCK=1.  Returns the number of workgroups written (0: not recorded).
int desc_debug_wg_clock(desc_pgd* h, uint64_t* out, int32_t cap) {
    if (!h || !out) return fail(DESC_ERR_INVALID, "NULL argument");
    if (!h->d_wg_clock || !h->band_ok) return 0;
    if (set_device(h)) return 0;
    const int nwg = std::min(cap, h->band_grid);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return 0;
    if (hipMemcpy(out, h->d_wg_clock, sizeof(uint64_t) * 2 * (size_t)nwg, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    if (2 * (int64_t)cap >= 3 * (int64_t)h->band_grid && nwg == h->band_grid &&          // room in out[2 * cap] for a third word per workgroup: its shader-clock cycles, at out[2 * nwg + w]
        hipMemcpy(out + 2 * (size_t)nwg, h->d_wg_clock + 2 * (size_t)nwg, sizeof(uint64_t) * (size_t)nwg, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return nwg;
}

// Diagnostics (tools/wg_clock.py): what the piece scheduler gave every workgroup of the band sweep -- out[4 * w + {0,1,2,3}] = cycles,
// segments, pieces, CSR entries of the band rows its pieces load.  Returns the number of workgroups.
int desc_debug_wg_plan(desc_pgd* h, int64_t* out, int32_t cap) {
    return no_throw("desc_debug_wg_plan", [&]() -> int {
    if (!h || !out) return fail(DESC_ERR_INVALID, "NULL argument");
    if (!h->band_ok || !h->d_pieces) return 0;
    if (set_device(h)) return 0;
    const int G = std::min(cap, h->band_grid);
    hvec<int32_t> pp((size_t)h->band_grid + 1), cum((size_t)h->m_pos + 1);
    if (hipMemcpy(pp.data(), h->d_piece_ptr, sizeof(int32_t) * pp.size(), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    if (hipMemcpy(cum.data(), h->d_cum, sizeof(int32_t) * cum.size(), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    hvec<PieceDesc> pc((size_t)pp[h->band_grid]);
    if (!pc.empty() && hipMemcpy(pc.data(), h->d_pieces, sizeof(PieceDesc) * pc.size(), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    for (int w = 0; w < G; ++w) {
        int64_t cyc = 0, seg = 0, rows = 0;
        for (int q = pp[w]; q < pp[w + 1]; ++q) { cyc += cum[pc[q].seg_hi] - cum[pc[q].seg_lo]; seg += pc[q].seg_hi - pc[q].seg_lo; rows += pc[q].row_len; }
        out[4 * w] = cyc; out[4 * w + 1] = seg; out[4 * w + 2] = pp[w + 1] - pp[w]; out[4 * w + 3] = rows;
    }
    return G;
    });
}

// What the layout of this handle moves per iteration (bench.py: the floor of its own traffic, next to the 72-byte algorithmic count):
// out[0] = (cycle, endpoint) pairs read by the column sums, out[1] = pieces of the band sweep, out[2] = bands, out[3] = CSR entries of band
// rows loaded into the LDS per sweep, out[4] = local cycles, out[5] = local segments; then which path the column sums take (tests): out[6] = lanes per
// segment (colsum_cl), out[7] = nodes with a workgroup each (colsum_long), out[8] = nodes visited (colsum_nodes), out[9] = colsum_fx_bits -- zeros on
// the gather layout, which has no column-sum pass.  Returns the number of values written.
int desc_pgd_layout_stats(const desc_pgd* h, int64_t* out, int32_t cap) {
    if (!h || !out) return fail(DESC_ERR_INVALID, "NULL argument");
    const bool node = h->variant == VARIANT_NODE;
    const int64_t v[10] = {h->colsum_entries, h->n_pieces, h->n_bands, h->piece_row_entries, local_cycles(h), node ? h->seg_hi - h->seg_lo : h->m_pos,
                           node ? h->colsum_cl : 0, node ? h->colsum_long : 0, node ? h->colsum_nodes : 0, node ? h->colsum_fx_bits : 0};
    int k = 0;
    for (; k < 10 && k < cap; ++k) out[k] = v[k];
    return k;
}

// Diagnostics (tests): name and template arguments of the sweep kernel this handle launched last ("" before the first sweep).
const char* desc_debug_last_sweep(const desc_pgd* h) { return h ? h->last_sweep.c_str() : ""; }

// 1 once the device-side patience rule has fired (synchronises the handle's stream)
int desc_pgd_stopped(desc_pgd* h, int32_t* stopped) {
    if (!h || !stopped) return fail(DESC_ERR_INVALID, "NULL argument");
    int rc = set_device(h); if (rc) return rc;
    DevState st{};
    flush_finalize(h);
    if ((rc = shard_unpack_pending(h))) return rc;
    if (h->comm_stream) DESC_HIP(hipStreamSynchronize(h->comm_stream));
    DESC_HIP(hipStreamSynchronize(h->stream));
    DESC_HIP(hipMemcpy(&st, h->d_state, sizeof st, hipMemcpyDeviceToHost));      // synchronous: `st` is a stack slot
    *stopped = st.stop;
    return DESC_OK;
}

}  // extern "C"

// NODE layout of the PGD sweep (see pgd.hip): k_sweep_node and k_sweep_small, their instance tables and launchers, and the choice between
// them and the band sweep (sweep_band.hip).
#include "pgd_handle.h"

namespace desc {

// ===========================================================================
// NODE variant
// ===========================================================================

struct StreamRegs { uint4 pk; double2 w, d; };   // one 16-byte vector of each streamed array

// LDS image of one chunk.  Entry q' = (cycle - a0) where a0 = c0 & ~3 is the chunk's first
// cycle rounded down to a 16-byte boundary of the packed-word array, so that every
// streaming load is a 16-byte access.
struct alignas(16) ChunkBuf {
    double w[CHUNK_LDS], d[CHUNK_LDS];
    uint32_t pk[CHUNK_LDS];
};

// The sweep (dominant kernel).  512-thread persistent workgroups take chunks of consecutive
// segments (<= CHUNK_CAP cycles, <= 8 * 64/LPS segments) round-robin: at any moment the
// resident workgroups read one contiguous window of the streamed arrays (DRAM row-buffer
// locality; disjoint far-apart streams per workgroup measured ~half the bandwidth).
// pk, w and S0 of a chunk arrive with 16-byte loads, two chunks ahead, and are parked in a
// triple-buffered LDS image.  Everything per segment lives in the registers of the 16 lanes
// that own the segment (LPS lanes x E cycles per lane = 16x1, 16x2, 32x2, 32x4, 64x4 for segments of up to 16, 32, 64, 128, 256 cycles; a
// chunk = one pass of the 8 waves x 64/LPS lane groups): the lane group
// that will compute segment t of chunk c+1 loads its records, issues its row gathers
// (addresses from the packed words already parked in LDS) and keeps their sums until the
// arithmetic of chunk c+1; E cycles per lane, reductions = E in-lane adds + 4 DPP steps
// shared by the 4 segments of a wave; simplex threshold by Michelot's fixed point with a
// division-free comparison (same active set as the reference's sort-and-scan, :215-223);
// weights and S leave with 8-byte stores straight from registers (16 lanes x 8 B = 128
// contiguous bytes).  One workgroup barrier per chunk.
//   iteration c:  park stream(c+1) -> LDS[(c+1)%3] | barrier | gathers(c+1) | records(c+2),
//                 stream(c+3) | arithmetic(c) out of LDS[c%3] + registers | land gathers and
//                 records | stores(c)
// gfx950 retires loads AND stores through one in-order counter (vmcnt): every pipelined
// load is unconditional (clamped index instead of a branch) so the compiler can count
// them, and a load that is waited for after a store point would make the wave wait for the
// stores too, so gathers and records are consumed (landed) after the arithmetic but before
// the stores of the iteration that issued them.  Chunk descriptors are prefetched four
// chunks ahead with one scalar 16-byte load (constant cache: off vmcnt).
// (the Adam variant carries two more streamed values per cycle through the arithmetic: it gets the
//  register budget of 3 waves per SIMD instead of spilling)
template <int LPS, int E, int STEP>
__global__ __launch_bounds__(SWEEP_THREADS, STEP == DESC_STEP_HYBRID ? 3 : 4) void k_sweep_node(NodeSweepArgs a) {
    __shared__ ChunkBuf X[3];
    __shared__ double s_nv[MAX_SEG_CYCLES + 1];
    if (a.state->stop) return;
    constexpr int NT = SWEEP_THREADS;
    static_assert(NT == 512 && (LPS == 16 || LPS == 32 || LPS == 64) && LPS * E <= MAX_SEG_CYCLES, "8 waves x 64/LPS lane groups per chunk");
    static_assert(CHUNK_LDS / 2 <= NT, "one 16-byte vector of w per thread");
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    constexpr int SPW = 64 / LPS;                      // segments per wave: a chunk holds at most 8 * SPW segments
    const int grp = lane / LPS, r16 = lane % LPS;      // LPS lanes per segment, E cycles per lane
    const int ts = wv * SPW + grp;                     // segment slot of this lane group
    const int nb = gridDim.x, lb = blockIdx.x;         // chunks dealt round-robin (see k_sweep_node)
    const int nk = lb < a.nchunks ? (a.nchunks - lb + nb - 1) / nb : 0;
    double obj_acc = 0.0, chg_acc = 0.0;
    if (nk == 0) { block_partials(obj_acc, chg_acc, a.partials, lb); return; }
    if (tid <= MAX_SEG_CYCLES) s_nv[tid] = tid <= a.max_cnt ? a.nv_tab[tid] : 0.0;

    struct RecRaw { int b0, b1; EdgeInfo ei; int2 x; };
    struct Rec { int qb, cnt, rbi, rbj, sa, sb, seg; };   // qb: image entry of the segment's first cycle; sharded runs: seg = ta, sb = tb
    struct Gat { double sjk[E], ski[E], T1, T2, So; };
    struct Landed { double ss[E], T1, T2, So; };       // S(jk)+S(ki) per cycle, mirror sums, old S of the segment
    struct Carry { StreamRegs s; Landed g; Rec r; };

    // past the end every load is redirected to this workgroup's last chunk: harmless and branch-free
    auto desc_of = [&](int k) -> ChunkDesc { return uniform_load_desc(a.chunk_desc, lb + min(k, nk - 1) * nb); };
    auto load_rec = [&](const ChunkDesc d) -> RecRaw {
        const int t = d.l0 + min(ts, d.l1 - d.l0 - 1);
        RecRaw r;
        r.b0 = a.cum[t]; r.b1 = a.cum[t + 1]; r.ei = a.einfo[t];
        r.x = a.xt ? a.xt[t] : int2{0, 0};
        return r;
    };
    auto land_rec = [&](const ChunkDesc d, const RecRaw q) -> Rec {
        Rec r;
        r.qb = q.b0 - (d.c0 & ~3);
        r.cnt = ts < d.l1 - d.l0 ? q.b1 - q.b0 : 0;
        r.rbi = q.ei.rb_i; r.rbj = q.ei.rb_j; r.sa = q.ei.slot_a; r.sb = a.xt ? q.x.y : q.ei.slot_b;
        r.seg = q.x.x;
        return r;
    };
    auto load_stream = [&](const ChunkDesc d) -> StreamRegs {   // 16-byte loads; image entry 0 = cycle a0 = c0 & ~3
        const int a0 = d.c0 & ~3, last = d.c1 - 1 - a0;
        const int v2 = min(tid, last >> 1), v4 = min(tid, last >> 2);
        StreamRegs sr;
        sr.w = *reinterpret_cast<const double2*>(a.w_old + a0 + 2 * (int64_t)v2);
        sr.d = *reinterpret_cast<const double2*>(a.S0 + a0 + 2 * (int64_t)v2);
        sr.pk = *reinterpret_cast<const uint4*>(a.pk + a0 + 4 * (int64_t)v4);
        return sr;
    };
    auto park = [&](const ChunkDesc d, const StreamRegs sr, ChunkBuf& xb) {
        const int last = d.c1 - 1 - (d.c0 & ~3);
        if (tid <= (last >> 1)) { *reinterpret_cast<double2*>(&xb.w[2 * tid]) = sr.w; *reinterpret_cast<double2*>(&xb.d[2 * tid]) = sr.d; }
        if (tid <= (last >> 2)) *reinterpret_cast<uint4*>(&xb.pk[4 * tid]) = sr.pk;
    };
    auto issue_gathers = [&](const Rec r, const ChunkBuf& xb) -> Gat {
        Gat g;
#pragma unroll
        for (int e = 0; e < E; ++e) {                // unconditional: idle lanes repeat the segment's first cycle
            const int idx = r16 + LPS * e;
            const uint32_t p = xb.pk[r.qb + (idx < r.cnt ? idx : 0)];
            const int si = r.rbi + (int)(p & 0x7FFFu), sj = r.rbj + (int)((p >> 16) & 0x7FFFu);
            g.sjk[e] = a.S_old[sj]; g.ski[e] = a.S_old[si];
        }
        const int ta = a.xt ? r.seg : r.sa, tb = r.sb;
        g.T1 = a.Tfull[ta];                      // column j of node i = sum(wijk(IKJ(mask)))  (:189)
        g.T2 = a.Tfull[tb];                      // column i of node j = sum(wijk(JKI(mask)))  (:190)
        g.So = a.S_old[r.sa];
        return g;
    };

    // one pipeline iteration: chunk k of this workgroup is computed; c.s = stream registers of
    // chunk k+1, c.g = gathers of chunk k, c.r = records of chunk k+1; r0 = records of chunk k
    auto iterate = [&](int k, const Carry c, const Rec r0, const ChunkDesc d0, const ChunkDesc d1, const ChunkDesc d2,
                       const ChunkDesc d3) -> Carry {
        Carry o;
        Gat gn;
        ChunkBuf& xc = X[k % 3];
        ChunkBuf& xn = X[(k + 1) % 3];
        park(d1, c.s, xn);
        __syncthreads();
        gn = issue_gathers(c.r, xn);
        const RecRaw q2 = load_rec(d2);
        o.s = load_stream(d3);
        // ---- arithmetic of chunk k
        const int a0 = d0.c0 & ~3;
        const int cnt = r0.cnt;
        const double T1 = fx_to_double(c.g.T1, a.fx_inv), T2 = fx_to_double(c.g.T2, a.fx_inv), nv = cnt > 0 ? s_nv[cnt] : 0.0;
        double ws[E];
        uint32_t okm = 0;
        double part = 0.0;
        // waves whose four lane groups own no segment of this chunk skip the arithmetic (wave-uniform)
        if (__ballot(cnt > 0) != 0ull) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int idx = r16 + LPS * e;
                const bool ok = idx < cnt;
                const int q = r0.qb + idx;
                uint32_t p = 0; double w = 0.0, d = 0.0;
                if (ok) { p = xc.pk[q]; w = xc.w[q]; d = xc.d[q]; okm |= 1u << e; }
                const double ss = c.g.ss[e];                                                         // S(jk)+S(ki)
                obj_acc += w * ss;                                                                   // :233, one sweep late
                const double g = ss + (((p & 0x8000u) ? T1 : 0.0) + ((p & 0x80000000u) ? T2 : 0.0)) * d;   // :193
                ws[e] = g;
                part += ok ? g * nv : 0.0;
            }
            const double dot = group_sum<LPS>(part);                                                    // :199-201
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int q = r0.qb + r16 + LPS * e;
                const double g = ws[e] - dot * nv;
                ws[e] = ((okm >> e) & 1u) ? apply_step<STEP>(a.st, xc.w[q], g, (int64_t)a0 + q) : 0.0;   // :207
            }
            // simplex projection threshold (:215-223), Michelot fixed point; the comparison
            // ws*na > s-1 is ws > (s-1)/na without a division per pass
            uint32_t act = okm;
            double s1v = 0.0; int na = 1;
            for (;;) {
                double sp = 0.0;
#pragma unroll
                for (int e = 0; e < E; ++e) sp += ((act >> e) & 1u) ? ws[e] : 0.0;
                s1v = group_sum<LPS>(sp) - 1.0;
                if (LPS == 16) na = max(group16_sum((int)__popc(act)), 1);
                else {                                 // wider groups: count by ballots (scalar popcounts)
                    na = 0;
#pragma unroll
                    for (int e = 0; e < E; ++e) na += group_count<LPS>((act >> e) & 1u, lane);
                    na = max(na, 1);
                }
                const double nad = (double)na;
                uint32_t keep = 0;
#pragma unroll
                for (int e = 0; e < E; ++e) keep |= (((act >> e) & 1u) && ws[e] * nad > s1v) ? 1u << e : 0u;
                const bool changed = keep != act;
                act = keep;
                if (!__any(changed)) break;
            }
            const double T = s1v / (double)na;
            double sn = 0.0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double wn = fmax(ws[e] - T, 0.0);                                              // :224
                ws[e] = wn;
                if ((okm >> e) & 1u) sn += wn * xc.d[r0.qb + r16 + LPS * e];
            }
            part = group_sum<LPS>(sn);                                                                  // :229
        }
        // gathers of chunk k+1 and records of chunk k+2 are consumed before this iteration's stores
        // (see the header); the gathers shrink to their sums
#pragma unroll
        for (int e = 0; e < E; ++e) o.g.ss[e] = gn.sjk[e] + gn.ski[e];
        o.g.T1 = gn.T1; o.g.T2 = gn.T2; o.g.So = gn.So;
        o.r = land_rec(d2, q2);
        // pin the landing here: without it the scheduler sinks these adds below the stores
#pragma unroll
        for (int e = 0; e < E; ++e) asm volatile("" : "+v"(o.g.ss[e]));
        asm volatile("" : "+v"(o.g.T1), "+v"(o.g.T2), "+v"(o.g.So));
        asm volatile("" : "+v"(o.r.qb), "+v"(o.r.cnt), "+v"(o.r.rbi), "+v"(o.r.rbj), "+v"(o.r.sa), "+v"(o.r.sb), "+v"(o.r.seg));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < E; ++e)
            if ((okm >> e) & 1u) a.w_new[(int64_t)a0 + r0.qb + r16 + LPS * e] = ws[e];
        if (cnt > 0 && r16 == 0) {
            chg_acc += fabs(part - c.g.So);                                                      // :232
            // sharded runs: only the all-gather slice is written; k_unpack_S scatters S of every edge, this rank's included
            if (a.s_slice) a.s_slice[r0.seg] = part;
            else { a.S_new[r0.sa] = part; a.S_new[r0.sb] = part; }
        }
        return o;
    };

    // ---- prologue: chunk 0 parked and its gathers in flight, streams of chunks 1 and 2 in flight
    ChunkDesc D0 = desc_of(0), D1 = desc_of(1), D2 = desc_of(2), D3 = desc_of(3);
    Rec R0;
    Carry CA, CB;
    {
        const RecRaw q0 = load_rec(D0);
        const StreamRegs s0 = load_stream(D0);
        const RecRaw q1 = load_rec(D1);
        CA.s = load_stream(D1);                  // CA: consumed by even iterations
        CB.s = load_stream(D2);
        R0 = land_rec(D0, q0);
        park(D0, s0, X[0]);
        __syncthreads();
        const Gat g0 = issue_gathers(R0, X[0]);
#pragma unroll
        for (int e = 0; e < E; ++e) CA.g.ss[e] = g0.sjk[e] + g0.ski[e];
        CA.g.T1 = g0.T1; CA.g.T2 = g0.T2; CA.g.So = g0.So;
        CA.r = land_rec(D1, q1);
    }
    // Two iterations per trip (the register sets alternate).  The second one always runs -- with
    // an odd number of chunks it computes nothing (cnt = 0) -- so that the compiler sees one
    // straight-line loop body and can count the loads in flight across the back edge.
    for (int k = 0; k < nk; k += 2) {
        {
            const ChunkDesc Dn = desc_of(k + 4);
            const Carry o = iterate(k, CA, R0, D0, D1, D2, D3);       // parks CA.s (chunk k+1), consumes CA.g (chunk k)
            R0 = CA.r; CB.g = o.g; CB.r = o.r; CA.s = o.s;            // CA.s now streams chunk k+3
            D0 = D1; D1 = D2; D2 = D3; D3 = Dn;
        }
        {
            if (k + 1 >= nk) R0.cnt = 0;
            const ChunkDesc Dn = desc_of(k + 5);
            const Carry o = iterate(k + 1, Carry{CB.s, CB.g, CB.r}, R0, D0, D1, D2, D3);
            R0 = CB.r; CA.g = o.g; CA.r = o.r; CB.s = o.s;
            D0 = D1; D1 = D2; D2 = D3; D3 = Dn;
        }
    }
    block_partials(obj_acc, chg_acc, a.partials, lb);
}

// SMALL graphs (round 4; the reference's own demo sizes, Demo/compare_algorithms.m:10: n = 100-200, configs[0]): an iteration of a few hundred
// thousand cycles is not bandwidth- but latency-bound -- k_sweep_node's staged chunk pipeline is a chain of ~6 dependent memory round trips for one
// chunk per workgroup (C1: 11.7 us per sweep for ~1 us of traffic).  Here a lane group of G lanes takes a whole segment (one cycle per lane) straight
// from global memory: records -> packed words / weights / S0 -> the gathers of S and the mirror sums -> arithmetic -> stores, three dependent round
// trips.  Same per-segment arithmetic as the gather layout's k_sweep (group reductions over G lanes, Michelot threshold), on the node layout's arrays.
template <int G, int STEP>
__global__ __launch_bounds__(256) void k_sweep_small(NodeSweepArgs a, int n_seg) {
    if (a.state->stop) return;
    constexpr int EPW = 64 / G;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sub = lane / G, gl = lane % G;
    double obj_acc = 0.0, chg_acc = 0.0;
    for (int l0 = ((int)blockIdx.x * 4 + wv) * EPW; l0 < n_seg; l0 += (int)gridDim.x * 4 * EPW) {
        const int l = l0 + sub;
        const bool seg_ok = l < n_seg;
        int base = 0, cnt = 0;
        EdgeInfo ei{0, 0, 0, 0};
        if (seg_ok) { base = a.cum[l]; cnt = a.cum[l + 1] - base; ei = a.einfo[l]; }
        const bool act0 = gl < cnt;
        const int64_t c = (int64_t)base + gl;
        uint32_t p = 0; double w = 0.0, d = 0.0, ssum = 0.0;
        if (act0) {
            p = a.pk[c]; w = a.w_old[c]; d = a.S0[c];
            ssum = a.S_old[ei.rb_j + (int)((p >> 16) & 0x7FFFu)] + a.S_old[ei.rb_i + (int)(p & 0x7FFFu)];          // S(jk) + S(ki)
        }
        double T1 = 0.0, T2 = 0.0, So = 0.0;
        if (seg_ok) { T1 = fx_to_double(a.Tfull[ei.slot_a], a.fx_inv); T2 = fx_to_double(a.Tfull[ei.slot_b], a.fx_inv); So = a.S_old[ei.slot_a]; }
        obj_acc += w * ssum;                                                                                     // :233, one sweep late
        double g = ssum + (((p & 0x8000u) ? T1 : 0.0) + ((p & 0x80000000u) ? T2 : 0.0)) * d;                     // :193
        const double nv = act0 ? a.nv_tab[cnt] : 0.0;
        const double dot = group_sum<G>(act0 ? g * nv : 0.0);                                                    // :199-201
        g = g - dot * nv;
        const double ws = act0 ? apply_step<STEP>(a.st, w, g, c) : 0.0;                                          // :207
        const double T = simplex_threshold<G>(ws, act0, lane);                                                   // :215-223
        const double wn = act0 ? fmax(ws - T, 0.0) : 0.0;                                                        // :224
        const double snew = group_sum<G>(wn * d);                                                                // :229
        if (act0) a.w_new[c] = wn;
        if (seg_ok && cnt > 0 && gl == 0) {
            chg_acc += fabs(snew - So);                                                                          // :232
            a.S_new[ei.slot_a] = snew; a.S_new[ei.slot_b] = snew;
        }
    }
    block_partials(obj_acc, chg_acc, a.partials, blockIdx.x);
}

namespace {

// node layout: lanes per segment x cycles per lane >= longest segment
// (33..64 cycles: 32 lanes x 2 cycles keeps all 8 waves of the workgroup busy in the arithmetic --
//  measured 2 % faster than 16 lanes x 4 cycles at C2 and C4)
template <int LPS, int E>
constexpr SweepInst<NodeSweepArgs> node_inst() { return {{LPS, E}, SWEEP_THREADS, {k_sweep_node<LPS, E, DESC_STEP_CONSTANT>, k_sweep_node<LPS, E, DESC_STEP_HYBRID>}}; }
// k_sweep_small: G lanes per segment (small_ok: segments of at most 64 cycles)
template <int G>
constexpr SweepInst<NodeSweepArgs, int> small_inst() { return {{G, 0}, 256, {k_sweep_small<G, DESC_STEP_CONSTANT>, k_sweep_small<G, DESC_STEP_HYBRID>}}; }
const SweepInst<NodeSweepArgs, int> SMALL_INSTS[] = {small_inst<16>(), small_inst<32>(), small_inst<64>()};

}  // namespace

const SweepInst<NodeSweepArgs> NODE_INSTS[] = {node_inst<16, 1>(), node_inst<16, 2>(), node_inst<32, 2>(), node_inst<32, 4>(), node_inst<64, 4>()};
const SweepInst<NodeSweepArgs>* node_inst_of(SweepShape sh) { return sweep_inst(NODE_INSTS, sh); }      // for setup_node's occupancy query (pgd_layout.hip)
SweepShape node_shape(int c) { return {c <= 32 ? 16 : c <= 128 ? 32 : 64, c <= 16 ? 1 : c <= 64 ? 2 : 4}; }      // 16 x 1, 16 x 2, 32 x 2, 32 x 4 or 64 x 4: each has its entry
std::string node_prefix(SweepShape sh) { return inst_name("k_sweep_node<%d,%d,", sh.lps, sh.E); }
SweepShape small_shape(int c) { return {c <= 16 ? 16 : c <= 32 ? 32 : 64, 0}; }      // 16, 32 or 64: each has its entry
std::string small_prefix(SweepShape sh) { return inst_name("k_sweep_small<%d,", sh.lps); }

namespace {

int launch_node(desc_pgd* h, const NodeSweepArgs& a, bool adam) {
    const auto* k = sweep_inst(NODE_INSTS, node_shape(h->max_cnt));
    if (!k) return DESC_ERR_STATE;
    h->last_sweep = node_prefix(k->sh) + inst_name("%d>%s", STEP_OF[adam], a.xt ? " sharded" : "");
    hipLaunchKernelGGL(k->kern[adam], dim3(h->grid), dim3(k->NT), 0, h->stream, a);
    return DESC_OK;
}

int launch_small(desc_pgd* h, const NodeSweepArgs& a, bool adam) {
    const auto* k = sweep_inst(SMALL_INSTS, small_shape(h->max_cnt));
    if (!k) return DESC_ERR_STATE;
    h->last_sweep = small_prefix(k->sh) + inst_name("%d>", STEP_OF[adam]);
    hipLaunchKernelGGL(k->kern[adam], dim3(h->small_grid), dim3(k->NT), 0, h->stream, a, (int)(h->seg_hi - h->seg_lo));
    return DESC_OK;
}

}  // namespace

int launch_sweep_node_layout(desc_pgd* h, const NodeSweepArgs& a, bool adam, int part) {
    if (h->small_ok && a.partials == h->d_partials) return launch_small(h, a, adam);      // the plain one-rank path only
    if (adam ? band_adam_ok(h) : h->band_ok) return launch_band(h, a, adam, part);
    return launch_node(h, a, adam);
}
// workgroups (= partial pairs) of the sweep kernel that serves this step kind
int sweep_parts(const desc_pgd* h, bool adam, bool plain_path) {
    if (plain_path && h->variant == VARIANT_NODE && h->small_ok) return h->small_grid;
    return h->variant == VARIANT_NODE && (adam ? band_adam_ok(h) : h->band_ok) ? h->band_grid + h->band_ntail : h->grid;
}

}  // namespace desc

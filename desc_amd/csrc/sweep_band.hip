// BAND sweep on the node layout (see pgd.hip): k_sweep_band, its two instance tables and its launcher.
#include "pgd_handle.h"

namespace desc {

// ===========================================================================
// BAND sweep: the same arithmetic with the i-rows of S in the LDS
// ===========================================================================
// k_sweep_node is bound by L1-miss sector traffic: every segment gathers ~cnt values out of row i of Sfull
// (8 useful bytes per 64-byte sector, a different row for every segment of a chunk).  Here the nodes are cut
// into bands whose CSR rows fit the LDS of one CU together (<= row_cap doubles: 36 rows at C2, 18 at C4 / C5);
// the edges keep the (band(i), j, i) order, every workgroup owns ONE contiguous range of segments (equal cycle
// counts; pure streaming measured no penalty for contiguous ranges -- tools/probes/stream_probe.hip), split into
// "pieces" at band boundaries, loads the piece's band rows once (coalesced) and serves S({k,i}) and the segment's
// old S from the LDS.  S({j,k}) stays a gather through L1: consecutive segments of a band share j.
// 1024 threads = 16 waves per workgroup (one workgroup per CU); no barrier inside a piece.  A wave takes
// SPW = 64/LPS consecutive segments per iteration; its software pipeline keeps, per lane group,
//   records (cum, EdgeInfo: scalar loads, off vmcnt)  4 iterations ahead,
//   the streamed pk / w / S0 of its cycles            3 iterations ahead (registers, 4 rotating sets),
//   the gathers of S({j,k}), T1, T2 (+ LDS reads)     1 iteration ahead (2 sets),
// issued in the order gathers -> stream -> arithmetic -> stores: loads and stores retire through one in-order
// counter on gfx950, so everything an iteration waits for was issued before the previous iteration's stores.
// BUFFER instructions (round 3).  The band sweep and the column sums address global memory as `descriptor in SGPRs + 32-bit byte offset per
// lane` (buffer_load / buffer_store ... offen) instead of a 64-bit address per lane (global_load / global_store): half the address data per
// instruction on the way to the address unit -- the busiest unit of the CU in this kernel (TA_BUSY 76 % at C4, section 5 of DESIGN.md) -- and no
// 64-bit address arithmetic (v_lshl_add_u64, sign extensions: 12 % of the VALU instructions of an iteration).  Measured, rocprofv3 averages in
// one call (profiles/r03_buffer_instructions.txt): only the S({j,k}) gathers C4 1171 -> 1119 us; + T1/T2 and the S stores 1122; + the three
// streams and the weight stores 1084-1091 (-7.2 %); C5 1737 -> 1670-1682, C3 105.0 -> 100.4, C2 110.8 -> 107.8.  Cache-policy bits on the
// gathers (same file): nt 1873 us, sc1 / sc0 sc1 1253 us -- no.  Offsets are 32 bits: the descriptors of the per-cycle arrays are rebuilt per
// piece with the piece's first cycle as base (any m_cycle), the CSR-aligned arrays (2m doubles) must stay below 4 GiB (setup_node: else no band sweep).
// Out-of-range offsets read 0 and store nothing (num_records) instead of faulting.  (The round-2 global-load forms are in the history, tree ca0abdf.)
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
template <class T> __device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const T* p, uint32_t bytes = 0xFFFFFFFFu) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, bytes, 0x00020000);          // raw buffer (stride 0), 32-bit data format
}
__device__ __forceinline__ double buf_load_f64(__amdgpu_buffer_rsrc_t rs, uint32_t off) {
    const u32x2_t v = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)off, 0, 0);
    double d; __builtin_memcpy(&d, &v, 8); return d;
}
__device__ __forceinline__ uint32_t buf_load_u32(__amdgpu_buffer_rsrc_t rs, uint32_t off) { return __builtin_amdgcn_raw_buffer_load_b32(rs, (int)off, 0, 0); }
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void buf_load_f64x2(__amdgpu_buffer_rsrc_t rs, uint32_t off, double& a0, double& a1) {      // 16 bytes, 8-byte aligned
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0);
    const u32x2_t lo = {v.x, v.y}, hi = {v.z, v.w};
    __builtin_memcpy(&a0, &lo, 8); __builtin_memcpy(&a1, &hi, 8);
}
__device__ __forceinline__ void buf_load_u32x2(__amdgpu_buffer_rsrc_t rs, uint32_t off, uint32_t& a0, uint32_t& a1) {
    const u32x2_t v = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)off, 0, 0);
    a0 = v.x; a1 = v.y;
}
__device__ __forceinline__ void buf_store_f64x2(__amdgpu_buffer_rsrc_t rs, uint32_t off, double d0, double d1) {
    u32x2_t lo, hi; __builtin_memcpy(&lo, &d0, 8); __builtin_memcpy(&hi, &d1, 8);
    const u32x4_t v = {lo.x, lo.y, hi.x, hi.y};
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, (int)off, 0, 0);
}
__device__ __forceinline__ void buf_store_f64(__amdgpu_buffer_rsrc_t rs, uint32_t off, double d) {
    u32x2_t v; __builtin_memcpy(&v, &d, 8);
    __builtin_amdgcn_raw_buffer_store_b64(v, rs, (int)off, 0, 0);
}

struct BandSweepArgs {
    NodeSweepArgs n;
    const PieceDesc* pieces;
    const int32_t* piece_ptr;      // grid + 1
    int32_t row_cap;
    unsigned long long* wg_clock;  // diagnostics (DESC_DEBUG_WGCLOCK=1; else NULL): per workgroup {start, end} of the constant 100 MHz clock
    // Dynamic tail (round 3): the last few per cent of the sweep's work are not in any workgroup's list but in a shared queue of small pieces
    // pieces[tail_first .. tail_first + n_tail), handed out by tickets to whichever workgroup has finished its list (the lists are balanced by
    // a cost model; the workgroups' real times differ by +-5 %).  Every tail piece has its own pair of partials (slot gridDim.x + ticket), so
    // the objective and |dS| sums do not depend on who took which piece.  *ticket is zeroed by the column-sum launch that precedes a sweep.
    int32_t tail_first, n_tail;
    int32_t* ticket;
};

__device__ __forceinline__ PieceDesc uniform_load_piece(const PieceDesc* p, int i) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    typedef const v4i __attribute__((address_space(4)))* cptr_t;
    const v4i v = ((cptr_t)(unsigned long long)p)[i];
    return PieceDesc{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ EdgeInfo uniform_load_einfo(const EdgeInfo* p, int i) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    typedef const v4i __attribute__((address_space(4)))* cptr_t;
    const v4i v = ((cptr_t)(unsigned long long)p)[i];
    return EdgeInfo{v.x, v.y, v.z, v.w};
}

template <int LPS, int E, int STEP, int NT, bool XT = false>      // XT: sharded run (exchange positions {ta, tb} per segment; its own instances keep
__global__ __launch_bounds__(NT, 1) void k_sweep_band(BandSweepArgs b) {     // the extra records out of the one-GPU kernels' scalar registers)
    extern __shared__ double s_dyn[];                  // [row_cap] band rows of S_old, then the nv table
    const NodeSweepArgs& a = b.n;
    double* s_rows = s_dyn;
    double* s_nv = s_dyn + b.row_cap;
    __shared__ double s_part[2][NT / 64];
    // segments of up to 64 cycles: 1024 threads (16 waves, <= 128 VGPRs each); up to 256 cycles (4 cycles per lane: twice the
    // registers per pipeline stage) and the Adam plugin (its two moments are two more streams in and out): 512 threads (8 waves, <= 256 VGPRs).
    static_assert((LPS == 8 || LPS == 16 || LPS == 32 || LPS == 64) && LPS * E <= MAX_SEG_CYCLES && (NT == 512 || NT == 1024) && (STEP != DESC_STEP_HYBRID || NT == 512), "band sweep instances");
    constexpr bool ADAM = STEP == DESC_STEP_HYBRID;
    constexpr int EA = ADAM ? E : 1;
    if (a.state->stop) return;
    constexpr int NW = NT / 64, SPW = 64 / LPS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = lane / LPS, rr = lane % LPS;
    if (tid <= MAX_SEG_CYCLES) s_nv[tid] = tid <= a.max_cnt ? a.nv_tab[tid] : 0.0;
    double obj_acc = 0.0, chg_acc = 0.0;

    constexpr bool VREC = SPW > 4;         // (for every shape, as buffer loads: C4 +4.7 %, C5 +3.6 %, C2 +2 % -- the scalar loads keep the records out of the address unit) eight segments per wave: their records would not fit the SGPRs -- per-lane vector loads instead
    struct RecRaw { int c0[VREC ? 1 : SPW], c1[VREC ? 1 : SPW]; EdgeInfo ei[VREC ? 1 : SPW]; int xa[XT ? (VREC ? 1 : SPW) : 1], xb[XT ? (VREC ? 1 : SPW) : 1]; int t0; };      // wave-uniform (SGPRs); VREC: this lane group's record (VGPRs)
    struct Rec { int c0, cnt, rbi, rbj, sa, sb, seg; };                   // this lane group's segment; sharded runs: seg = ta, sb = tb (exchange positions)
    // Which cycles of its segment a lane owns.  Round 2: rr + LPS * e (every stream instruction reads one contiguous run of 8-byte words).
    // Round 3 (PAIR): the adjacent pairs 2 rr + 2 LPS * (e / 2) + {0, 1}, so that the 8-byte streams (old weights, S0, Adam moments) are read
    // 16 bytes per lane: the CU's address unit takes 16.4 cycles for a contiguous 8-byte-per-lane load and 16.3 for a 16-byte one
    // (tools/probes/gather_probe.hip, profiles/r03_gather_probe.txt), i.e. half the cycles per byte.  The packed words become 8-byte loads
    // (16.4 cycles for two cycles' worth instead of 2 x 6.2), the weight stores 16-byte stores (43.6 = 2 x 21.9: no change).
    // Only the constant / piecewise-step shapes for segments of up to 64 cycles (LPS <= 16: what the BASELINE workloads run).  Measured on the others:
    // unsampled C5 (<64,4>) 8.05 -> 7.89 ms; the Adam instances (<32,2> at C2 / C4) no gain (2.19 -> 2.27 ms at C4, 0.251 -> 0.267 at C2) -- both
    // keep the round-2 map, and with it results bitwise equal to k_sweep_node's (which two tests assert).
    constexpr bool PAIR = (E % 2 == 0) && LPS <= 16 && !ADAM;
    // (four adjacent cycles per lane -- the packed words as ONE 16-byte load -- measured on top: C4 1025-1054 vs 989-1034 us, C2 +3 %: not adopted)
    auto cidx = [&](int e) { return PAIR ? 2 * rr + (e & 1) + 2 * LPS * (e >> 1) : rr + LPS * e; };
    struct Str { uint32_t pk[E]; double w[E], d[E], am[EA], av[EA]; };     // am / av: HybridGradient.m_t / v_t (Adam only)
    struct Gat { double sj[E], si[E], T1, T2, So; };

    const int p0 = uniform_load(b.piece_ptr, blockIdx.x), p1 = uniform_load(b.piece_ptr, blockIdx.x + 1);
    unsigned long long wg_c0 = 0;
    if (b.wg_clock && tid == 0) { b.wg_clock[2 * blockIdx.x] = wall_clock64(); wg_c0 = clock64(); }
    __shared__ int s_ticket;
    // deterministic workgroup partials of what has been accumulated since the last flush -> pair `slot`
    auto flush_partials = [&](int slot) {
        const double o1 = group_sum<64>(obj_acc), c1 = group_sum<64>(chg_acc);
        __syncthreads();
        if (lane == 0) { s_part[0][wv] = o1; s_part[1][wv] = c1; }
        __syncthreads();
        if (tid == 0) {
            double o = 0.0, c = 0.0;
            for (int k = 0; k < NW; ++k) { o += s_part[0][k]; c += s_part[1][k]; }
            a.partials[2 * slot] = o;
            a.partials[2 * slot + 1] = c;
        }
        obj_acc = 0.0; chg_acc = 0.0;
    };
    // num_records = the arrays' real lengths: an offset past the end reads 0 / stores nothing instead of touching a neighbouring block
#ifndef DESC_RSRC_UNBOUNDED          // A/B builds only: 1 = the round-3 descriptors (num_records 0xFFFFFFFF)
#define DESC_RSRC_UNBOUNDED 0
#endif
    const uint32_t nb_csr = DESC_RSRC_UNBOUNDED ? 0xFFFFFFFFu : a.csr_bytes, nb_t = DESC_RSRC_UNBOUNDED ? 0xFFFFFFFFu : a.t_bytes, nb_sl = DESC_RSRC_UNBOUNDED ? 0xFFFFFFFFu : a.slice_bytes;
    const __amdgpu_buffer_rsrc_t rs_S = make_rsrc(a.S_old, nb_csr), rs_T = make_rsrc(a.Tfull, nb_t), rs_Sn = make_rsrc(a.S_new, nb_csr);      // CSR-aligned: 2m doubles < 4 GiB
    const __amdgpu_buffer_rsrc_t rs_sl = XT ? make_rsrc(a.s_slice, nb_sl) : rs_Sn;                        // sharded runs: this rank's all-gather slice
    const __amdgpu_buffer_rsrc_t rs_cum = make_rsrc(a.cum, (a.seg_count + 1u) * 4u), rs_ei = make_rsrc(a.einfo, a.seg_count * 16u);          // per-lane records (VREC shapes only; C3 -1 %)
    int pc = p0, ticket = -1;
    for (;;) {
        if (ticket < 0 && pc >= p1) {                      // own list done: its partials, then the shared tail
            flush_partials(blockIdx.x);
            if (b.n_tail == 0) break;
            ticket = 0;
        }
        if (ticket >= 0) {
            if (tid == 0) s_ticket = atomicAdd(b.ticket, 1);
            __syncthreads();
            ticket = __builtin_amdgcn_readfirstlane(s_ticket);
            __syncthreads();
            if (ticket >= b.n_tail) break;
            pc = b.tail_first + ticket;
        }
        const PieceDesc pd = uniform_load_piece(b.pieces, pc);
        __syncthreads();                                   // every wave is done with the previous band's rows
        const int nit = (pd.seg_hi - pd.seg_lo + NW * SPW - 1) / (NW * SPW);
        // the piece's cycles are one contiguous range of the per-cycle arrays: Rec::c0 counts from its start
        const int c_lo = uniform_load(a.cum, pd.seg_lo);
        const uint32_t c_len = (uint32_t)(uniform_load(a.cum, pd.seg_hi) - c_lo) + 8u;           // + the 16-byte tail the arrays are padded by
        const __amdgpu_buffer_rsrc_t rs_pk = make_rsrc(a.pk + c_lo, c_len * 4u), rs_w = make_rsrc(a.w_old + c_lo, c_len * 8u),
                                     rs_d = make_rsrc(a.S0 + c_lo, c_len * 8u), rs_wn = make_rsrc(a.w_new + c_lo, c_len * 8u);
        __amdgpu_buffer_rsrc_t rs_am = rs_w, rs_av = rs_w, rs_amo = rs_wn, rs_avo = rs_wn;       // Adam moments (HybridGradient.m:28-35), read and written per cycle
        if constexpr (ADAM) {
            rs_am = make_rsrc(a.st.adam_m + c_lo, c_len * 8u); rs_av = make_rsrc(a.st.adam_v + c_lo, c_len * 8u);
            rs_amo = make_rsrc(a.st.adam_m_out + c_lo, c_len * 8u); rs_avo = make_rsrc(a.st.adam_v_out + c_lo, c_len * 8u);
        }

        auto load_raw = [&](int it) -> RecRaw {            // past the end: the piece's last segment, cnt = 0
            RecRaw q;
            q.t0 = pd.seg_lo + (it * NW + wv) * SPW;
            if constexpr (VREC) {
                const int t = min(q.t0 + grp, pd.seg_hi - 1);
                {
                    const u32x2_t cc = __builtin_amdgcn_raw_buffer_load_b64(rs_cum, t * 4, 0, 0);
                    const u32x4_t ee = __builtin_amdgcn_raw_buffer_load_b128(rs_ei, t * 16, 0, 0);
                    q.c0[0] = (int)cc.x; q.c1[0] = (int)cc.y;
                    q.ei[0].rb_i = (int)ee.x; q.ei[0].rb_j = (int)ee.y; q.ei[0].slot_a = (int)ee.z; q.ei[0].slot_b = (int)ee.w;
                }
                if constexpr (XT) { const int2 x = a.xt[t]; q.xa[0] = x.x; q.xb[0] = x.y; }
                return q;
            }
#pragma unroll
            for (int s2 = 0; s2 < SPW; ++s2) {
                const int t = min(q.t0 + s2, pd.seg_hi - 1);
                q.c0[s2] = uniform_load(a.cum, t); q.c1[s2] = uniform_load(a.cum, t + 1);
                q.ei[s2] = uniform_load_einfo(a.einfo, t);
                if constexpr (XT) { q.xa[s2] = uniform_load((const int32_t*)a.xt, 2 * t); q.xb[s2] = uniform_load((const int32_t*)a.xt, 2 * t + 1); }
            }
            return q;
        };
        auto land = [&](const RecRaw& q) -> Rec {
            Rec r{};
            if constexpr (VREC) {
                r.c0 = q.c0[0] - c_lo; r.cnt = q.t0 + grp < pd.seg_hi ? q.c1[0] - q.c0[0] : 0;
                r.rbi = q.ei[0].rb_i - pd.row_lo; r.rbj = q.ei[0].rb_j; r.sa = q.ei[0].slot_a; r.sb = XT ? q.xb[0] : q.ei[0].slot_b;
                r.seg = XT ? q.xa[0] : 0;
                return r;
            }
#pragma unroll
            for (int s2 = 0; s2 < SPW; ++s2)
                if (grp == s2) {
                    r.c0 = q.c0[s2] - c_lo; r.cnt = q.t0 + s2 < pd.seg_hi ? q.c1[s2] - q.c0[s2] : 0;
                    r.rbi = q.ei[s2].rb_i - pd.row_lo; r.rbj = q.ei[s2].rb_j; r.sa = q.ei[s2].slot_a; r.sb = XT ? q.xb[s2] : q.ei[s2].slot_b;
                    r.seg = XT ? q.xa[s2] : 0;
                }
            return r;
        };
        auto load_stream = [&](const Rec& r) -> Str {      // unconditional: idle lanes repeat a valid cycle of the segment
            Str x;
            if constexpr (PAIR) {
#pragma unroll
                for (int h = 0; h < E / 2; ++h) {
                    // the pair's first cycle, clamped into the segment; its second one may lie past the segment's end (an odd count, idle lanes):
                    // that is the next segment's first cycle or the arrays' padding -- readable, masked in compute; its packed word is replaced by
                    // the first one's, so that the gathers formed from it stay inside rows i and j
                    const int first = min(2 * rr + 2 * LPS * h, max(r.cnt, 1) - 1);
                    const uint32_t cr = (uint32_t)(r.c0 + first);
                    buf_load_u32x2(rs_pk, cr * 4u, x.pk[2 * h], x.pk[2 * h + 1]);
                    buf_load_f64x2(rs_w, cr * 8u, x.w[2 * h], x.w[2 * h + 1]);
                    buf_load_f64x2(rs_d, cr * 8u, x.d[2 * h], x.d[2 * h + 1]);
                    if (ADAM) { buf_load_f64x2(rs_am, cr * 8u, x.am[(2 * h) % EA], x.am[(2 * h + 1) % EA]); buf_load_f64x2(rs_av, cr * 8u, x.av[(2 * h) % EA], x.av[(2 * h + 1) % EA]); }
                    if (first + 1 >= r.cnt) x.pk[2 * h + 1] = x.pk[2 * h];
                }
                return x;
            }
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int cr = r.c0 + min(rr + LPS * e, max(r.cnt, 1) - 1);
                x.pk[e] = buf_load_u32(rs_pk, (uint32_t)cr * 4u); x.w[e] = buf_load_f64(rs_w, (uint32_t)cr * 8u); x.d[e] = buf_load_f64(rs_d, (uint32_t)cr * 8u);
                if (ADAM) { x.am[e % EA] = buf_load_f64(rs_am, (uint32_t)cr * 8u); x.av[e % EA] = buf_load_f64(rs_av, (uint32_t)cr * 8u); }
            }
            return x;
        };
        auto issue_gathers = [&](const Rec& r, const Str& x) -> Gat {
            Gat g;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const uint32_t p = x.pk[e];
                g.sj[e] = buf_load_f64(rs_S, (uint32_t)(r.rbj + (int)((p >> 16) & 0x7FFFu)) * 8u);      // S({j,k}): a gather inside row j (L1 / L2)
                g.si[e] = s_rows[r.rbi + (int)(p & 0x7FFFu)];                                              // S({k,i}): the band's rows in the LDS
            }
            const int ta = XT ? r.seg : r.sa, tb = r.sb;
                        // this and the single S store: C4 1059.5 -> 1045.8 / 1083 -> 1059 us, C2 within noise (profiles/r03_buffer_instructions.txt)
            g.T1 = buf_load_f64(rs_T, (uint32_t)((lane & 1) ? tb : ta) * 8u);
            g.T2 = 0.0;
            g.So = s_rows[r.sa - pd.row_lo];
            return g;
        };
        // arithmetic + stores of one segment group (DESC_PGD.m:193-233), everything in registers
        auto compute = [&](const Rec& r, const Str& x, const Gat& g0) {
            const int cnt = r.cnt;
            Gat g = g0;
            const double tconv = fx_to_double(g0.T1, a.fx_inv);       // this lane's load: T1 (even lanes) or T2 (odd lanes)
            g.T1 = dpp_mov_f64<0xA0>(tconv);        // quad_perm:[0,0,2,2]: the even lane's value = T1
            g.T2 = dpp_mov_f64<0xF5>(tconv);        // quad_perm:[1,1,3,3]: the odd lane's value = T2
            double ws[E], mo[EA], vo[EA];
            uint32_t okm = 0;
            double part = 0.0;
            if (__ballot(cnt > 0) != 0ull) {               // wave-uniform; no memory operation inside
                const double nv = cnt > 0 ? s_nv[cnt] : 0.0;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    // idle lanes (ok false) hold a copy of the segment's last cycle (load_stream clamps): what they compute from it is finite and
                    // discarded below (ws[e] = 0, no part in any sum), so only the sums mask them
                    const bool ok = cidx(e) < cnt;
                    const uint32_t p = x.pk[e];
                    const double w = ok ? x.w[e] : 0.0, d = x.d[e];
                    if (ok) okm |= 1u << e;
                    const double ss = g.sj[e] + g.si[e];                                                 // S(jk)+S(ki)
                    obj_acc += w * ss;                                                                   // :233, one sweep late
                    const double gr = ss + (((p & 0x8000u) ? g.T1 : 0.0) + ((p & 0x80000000u) ? g.T2 : 0.0)) * d;   // :193
                    ws[e] = gr;
                    part += ok ? gr * nv : 0.0;
                }
                const double dot = group_sum<LPS>(part);                                                 // :199-201
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const double gr = ws[e] - dot * nv;
                    if (ADAM) {                            // HybridGradient.m:28-35 (strategy 0): apply_step with the moments in registers
                        const double mt = (a.st.beta1 * x.am[e % EA]) + (1.0 - a.st.beta1) * gr;
                        const double vt = (a.st.beta2 * x.av[e % EA]) + (1.0 - a.st.beta2) * (gr * gr);
                        mo[e % EA] = mt; vo[e % EA] = vt;
                        const double cm = mt / a.st.bc1, cv = vt / a.st.bc2;
                        ws[e] = ((okm >> e) & 1u) ? x.w[e] + (-a.st.lr * cm / (sqrt(cv) + 1e-8)) : 0.0;
                    } else
                    ws[e] = ((okm >> e) & 1u) ? apply_step<STEP>(a.st, x.w[e], gr, 0) : 0.0;             // :207
                }
                uint32_t act = okm;                        // simplex threshold (:215-223), Michelot fixed point
                double s1v = 0.0; int na = 1;
                for (;;) {
                    double sp = 0.0;
#pragma unroll
                    for (int e = 0; e < E; ++e) sp += ((act >> e) & 1u) ? ws[e] : 0.0;
                    s1v = group_sum<LPS>(sp) - 1.0;
                    if (LPS == 8) na = max(group8_sum((int)__popc(act)), 1);
                    else if (LPS == 16) na = max(group16_sum((int)__popc(act)), 1);
                    else {
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
                    if ((okm >> e) & 1u) sn += wn * x.d[e];
                }
                part = group_sum<LPS>(sn);                                                               // :229
            }
            if constexpr (PAIR) {                      // 16-byte stores of the pairs; the last pair of an odd segment: its first cycle alone
#pragma unroll
                for (int h = 0; h < E / 2; ++h) {
                    const uint32_t off = (uint32_t)(r.c0 + cidx(2 * h)) * 8u;
                    const bool ok0 = (okm >> (2 * h)) & 1u, ok1 = (okm >> (2 * h + 1)) & 1u;
                    if (ok1) {
                        buf_store_f64x2(rs_wn, off, ws[2 * h], ws[2 * h + 1]);
                        if (ADAM) { buf_store_f64x2(rs_amo, off, mo[(2 * h) % EA], mo[(2 * h + 1) % EA]); buf_store_f64x2(rs_avo, off, vo[(2 * h) % EA], vo[(2 * h + 1) % EA]); }
                    } else if (ok0) {
                        buf_store_f64(rs_wn, off, ws[2 * h]);
                        if (ADAM) { buf_store_f64(rs_amo, off, mo[(2 * h) % EA]); buf_store_f64(rs_avo, off, vo[(2 * h) % EA]); }
                    }
                }
            } else
#pragma unroll
            for (int e = 0; e < E; ++e)
                if ((okm >> e) & 1u) {
                    buf_store_f64(rs_wn, (uint32_t)(r.c0 + rr + LPS * e) * 8u, ws[e]);
                    if (ADAM) { buf_store_f64(rs_amo, (uint32_t)(r.c0 + rr + LPS * e) * 8u, mo[e % EA]); buf_store_f64(rs_avo, (uint32_t)(r.c0 + rr + LPS * e) * 8u, vo[e % EA]); }
                }
            if (!XT && cnt > 0 && rr < 2) buf_store_f64(rs_Sn, (uint32_t)(rr == 0 ? r.sa : r.sb) * 8u, part);
            if (cnt > 0 && rr == 0) {
                chg_acc += fabs(part - g.So);                                                            // :232
                if constexpr (XT) buf_store_f64(rs_sl, (uint32_t)r.seg * 8u, part);       // sharded: k_unpack_S copies it into the CSR-aligned replica
            }
        };

        // ---- prologue: records 0..3, streams 0..2, gathers 0
        Rec R0, R1, R2, R3; Str S0, S1, S2, S3; Gat G0, G1;
        RecRaw Q;
        { const RecRaw q = load_raw(0); R0 = land(q); S0 = load_stream(R0); }
        { const RecRaw q = load_raw(1); R1 = land(q); S1 = load_stream(R1); }
        { const RecRaw q = load_raw(2); R2 = land(q); S2 = load_stream(R2); }
        Q = load_raw(3);
        // the band's rows of S_old -> LDS, while the first streams are in flight
        {
            // up to 19 loads in flight per thread: one batch for 1024 threads, two for 512 (38 at once cost the 64 x 4 instance 3.5 %)
            constexpr int RL = (BAND_ROW_CAP + 1023) / 1024;
            // 16 bytes per lane (half the address-unit cycles per byte, see PAIR): thread t takes the doubles 2 t, 2 t + 1 of every batch of 2 NT.
            // The clamped load of a one-entry band would end one double past the rows -- such a band (one node of degree 1, no triangle) never has a
            // segment and therefore never a piece; all the same rs_S carries the array's real length (the read returns 0) and the CSR-aligned arrays
            // are allocated two doubles longer.
            constexpr int RL2 = (RL + 1) / 2;
            for (int base = 0; base < pd.row_len; base += 2 * RL2 * NT) {
                double v0[RL2], v1[RL2];
#pragma unroll
                for (int u = 0; u < RL2; ++u)
                    buf_load_f64x2(rs_S, (uint32_t)(pd.row_lo + min(base + 2 * (u * NT + tid), max(pd.row_len - 2, 0))) * 8u, v0[u], v1[u]);
#pragma unroll
                for (int u = 0; u < RL2; ++u) {
                    const int t0 = base + 2 * (u * NT + tid);
                    if (t0 + 1 < pd.row_len) { s_rows[t0] = v0[u]; s_rows[t0 + 1] = v1[u]; }
                    else if (t0 < pd.row_len) s_rows[t0] = pd.row_len >= 2 ? v1[u] : v0[u];      // the row's last double: the clamped load ended on it
                }
            }
        }
        __syncthreads();
        G0 = issue_gathers(R0, S0);
        // one iteration: Ra/Sa/Ga = group g (computed), Rb/Sb = g+1 (gathers issued into Gb), Rd/Sd <- g+3
        auto step = [&](int g, const Rec& Ra, const Str& Sa, const Gat& Ga, const Rec& Rb, const Str& Sb, Gat& Gb, Rec& Rd, Str& Sd) {
            const RecRaw qn = load_raw(g + 4);
            Gb = issue_gathers(Rb, Sb);
            Rd = land(Q);
            Sd = load_stream(Rd);
            compute(Ra, Sa, Ga);
            Q = qn;
        };
        for (int g = 0; g < nit; g += 4) {                 // the tail iterations past nit compute nothing (cnt = 0)
            step(g,     R0, S0, G0, R1, S1, G1, R3, S3);
            step(g + 1, R1, S1, G1, R2, S2, G0, R0, S0);
            step(g + 2, R2, S2, G0, R3, S3, G1, R1, S1);
            step(g + 3, R3, S3, G1, R0, S0, G0, R2, S2);
        }
        if (ticket >= 0) flush_partials((int)gridDim.x + ticket);      // a tail piece: its own pair of partials
        else ++pc;
    }
    if (b.wg_clock && tid == 0) {
        b.wg_clock[2 * blockIdx.x + 1] = wall_clock64();
        b.wg_clock[2 * gridDim.x + blockIdx.x] = clock64() - wg_c0;          // shader-clock cycles of the same interval: the clock the box ran at
    }
}

namespace {

// Band sweep instances by the longest segment: lanes per segment x cycles per lane, threads per workgroup.
//   <= 16 cycles: 16 x 1, 1024     <= 32: 16 x 2, 512 (8 x 4, 512 on small graphs)     <= 64: 16 x 4, 512     <= 128: 32 x 4, 512     <= 256: 64 x 4, 512
// (33..64 cycles: 8 waves with 4 cycles per lane beat 16 waves of 32 x 2 by 5 % at C2 and C4 -- the DPP reductions are shared by four
//  segments per wave instead of two.  17..32 cycles: 8 lanes x 4 cycles, eight segments per wave with their records in per-lane vector
//  loads (they would spill the SGPRs), gains 4-5 % where S stays in the L2 (C3) and loses 1-2 % at C5; there 16 x 2 on 8 waves beats
//  the same shape on 16 waves by 2-4 % (12 waves: 1 %; 4 waves lose 7-22 % everywhere): fewer waves keep more of the j rows in the caches --
//  the PMC traffic of the C4 sweep fell from 6.2 to 5.6 GB with the 8-wave shape.)
// The Adam plugin: 512-thread instances (the moments ride in the stream sets) up to 64 cycles: 16 x 1, 16 x 2, 32 x 2.
template <int LPS, int E, int STEP, int NT>
constexpr SweepInst<BandSweepArgs> band_inst() { return {{LPS, E}, NT, {k_sweep_band<LPS, E, STEP, NT, false>, k_sweep_band<LPS, E, STEP, NT, true>}}; }
const SweepInst<BandSweepArgs> BAND_INSTS[] = {band_inst<16, 1, DESC_STEP_CONSTANT, 1024>(), band_inst<16, 2, DESC_STEP_CONSTANT, 512>(), band_inst<8, 4, DESC_STEP_CONSTANT, 512>(),
                                               band_inst<16, 4, DESC_STEP_CONSTANT, 512>(), band_inst<32, 4, DESC_STEP_CONSTANT, 512>(), band_inst<64, 4, DESC_STEP_CONSTANT, 512>()};
const SweepInst<BandSweepArgs> BAND_ADAM_INSTS[] = {band_inst<16, 1, DESC_STEP_HYBRID, 512>(), band_inst<16, 2, DESC_STEP_HYBRID, 512>(), band_inst<32, 2, DESC_STEP_HYBRID, 512>()};

}  // namespace

// Adam above 64 cycles: 4 cycles per lane + the moments do not fit the registers -- no band instance, k_sweep_node sweeps
bool band_adam_ok(const desc_pgd* h) { return h->band_ok && h->max_cnt <= 64; }
SweepShape band_shape(const desc_pgd* h, bool adam) {      // constant step: the six shapes of BAND_INSTS; Adam (at most 64 cycles): the three of BAND_ADAM_INSTS
    const int c = h->max_cnt;
    if (adam) return c <= 16 ? SweepShape{16, 1} : c <= 32 ? SweepShape{16, 2} : SweepShape{32, 2};
    if (c > 16 && c <= 32 && !h->band_jmajor) return SweepShape{8, 4};      // graphs whose S stays in the L2 (contiguous ranges)
    return c <= 16 ? SweepShape{16, 1} : c <= 32 ? SweepShape{16, 2} : c <= 64 ? SweepShape{16, 4} : c <= 128 ? SweepShape{32, 4} : SweepShape{64, 4};
}
const SweepInst<BandSweepArgs>* band_inst_of(const desc_pgd* h, bool adam) {
    return adam ? sweep_inst(BAND_ADAM_INSTS, band_shape(h, true)) : sweep_inst(BAND_INSTS, band_shape(h, false));
}
std::string band_prefix(SweepShape sh) { return inst_name("k_sweep_band<%d,%d,", sh.lps, sh.E); }
int launch_band(desc_pgd* h, const NodeSweepArgs& a, bool adam, int part) {
    const auto* k = band_inst_of(h, adam);
    if (!k) return DESC_ERR_STATE;
    // the plan of exchange part `part` (one-rank handles: the only one)
    BandSweepArgs b{a, h->d_pieces + h->xpiece_base[part], h->d_piece_ptr + h->xpiece_ptr_base[part], h->band_rows, h->d_wg_clock, h->xtail_first[part], h->xntail[part],
                    h->d_ticket + part};
    h->last_sweep = band_prefix(k->sh) + inst_name("%d,%d,%s>", STEP_OF[adam], k->NT, a.xt ? "XT" : "one-rank");
    hipLaunchKernelGGL(k->kern[a.xt != nullptr], dim3(h->band_grid), dim3(k->NT), h->band_lds, h->stream, b);
    return DESC_OK;
}

}  // namespace desc

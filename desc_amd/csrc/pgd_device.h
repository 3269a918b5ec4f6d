// Device-side text that more than one kernel unit of the PGD solver needs (pgd.hip, pgd_layout.hip, pgd_shard.hip, pgd_ext.hip,
// sweep_gather.hip, sweep_node.hip, sweep_band.hip): plain structs and __device__ __forceinline__ helpers only -- every __global__ kernel lives
// in exactly one .hip.
#pragma once

#include "device_utils.h"
#include "pgd_math.h"

namespace desc {

struct DevState {
    int32_t stop;          // 1 once the patience rule fired
    int32_t misses;        // DESC_PGD.m:181
    int32_t iters_run;     // iteration at which the loop broke
    int32_t final_parity;  // which double buffer holds the final iterate
    int32_t last_tested;   // last iteration whose stop test (:243-256) has been applied: a download between
                           // iterations evaluates the objective early, the next sweep must not count it again
};

// The mirror-weight sums travel as 64-bit fixed-point integers (k_colsum_node: order-independent adds; sharded runs reduce-scatter them as
// ncclInt64, so the totals -- and with them S_vec and the weights -- are bitwise the same for every number of ranks).  `t` holds the bits.
__device__ __forceinline__ double fx_to_double(double t, double fx_inv) { return (double)__double_as_longlong(t) * fx_inv; }

// deterministic workgroup partials (blockDim 256 or 512)
__device__ __forceinline__ void block_partials(double obj_acc, double chg_acc, double* partials, int lb) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    obj_acc = group_sum<64>(obj_acc);
    chg_acc = group_sum<64>(chg_acc);
    __shared__ double sh[16];
    if (lane == 0) { sh[wv] = obj_acc; sh[8 + wv] = chg_acc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double o = 0.0, c = 0.0;
        for (int k = 0; k < nw; ++k) { o += sh[k]; c += sh[8 + k]; }
        partials[2 * lb] = o;
        partials[2 * lb + 1] = c;
    }
}

// what a sweep on the gather layout is given (sweep_gather.hip)
struct SweepArgs {
    const int32_t* cum;       // m_pos+1
    const int32_t* pos_edge;  // m_pos
    const int32_t* e_jk;
    const int32_t* e_ki;
    const int32_t* ikj;
    const int32_t* jki;
    const double* S0;
    const double* w_old;
    double* w_new;
    const double* S_old;
    double* S_new;
    const double* nv_tab;     // nv_tab[c] = 1/sqrt(c)   (DESC_PGD.m:199)
    double* partials;         // [grid][2]: objective of the old iterate, sum |dS|
    const DevState* state;
    StepArgs st;
    int32_t m_pos;
};

// per edge-with-cycles, in device (band-major) order
struct EdgeInfo {
    int32_t rb_i;     // rowptr[i]
    int32_t rb_j;     // rowptr[j]
    int32_t slot_a;   // rowptr[i] + idx_i(j): this edge's slot in row i of Sfull / Tfull
    int32_t slot_b;   // rowptr[j] + idx_j(i): this edge's slot in row j
};
// packed per-cycle word: bits 0-14 idx_i(k), bit 15 cycle (ik;j) sampled (IKJ_appears, :113),
//                        bits 16-30 idx_j(k), bit 31 cycle (jk;i) sampled (JKI_appears, :124)


constexpr int SWEEP_THREADS = 512;

// first / end cycle and first / end segment of a chunk, one 16-byte scalar load
struct alignas(16) ChunkDesc { int32_t c0, c1, l0, l1; };
__device__ __forceinline__ ChunkDesc uniform_load_desc(const ChunkDesc* p, int i) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    typedef const v4i __attribute__((address_space(4)))* cptr_t;
    const v4i v = ((cptr_t)(unsigned long long)p)[i];
    return ChunkDesc{v.x, v.y, v.z, v.w};
}

struct NodeSweepArgs {
    const int32_t* cum;        // m_pos+1, device order
    const EdgeInfo* einfo;     // m_pos
    const uint32_t* pk;        // m_cycle
    const double* S0;
    const double* w_old;
    double* w_new;
    const double* S_old;       // Sfull, 2m
    double* S_new;
    const double* Tfull;       // 2m: Tfull[rowptr[v]+t] = sum_k w(v,k; nbr_t), masked; sharded runs: T1, T2 per owned segment
    const int2* xt;            // sharded runs (else NULL): per device-order segment {ta, tb}: Tfull (= the reduce-scattered sums of this rank) holds
                               // T1 of the segment at ta, T2 at tb (exchange layout: see k_xpos); ta is also its place in the all-gather slice
    double* s_slice;           // sharded runs: the new S of segment l goes to s_slice[ta] (this rank's all-gather slice)
    const double* nv_tab;
    double* partials;
    const DevState* state;
    const ChunkDesc* chunk_desc;   // nchunks: {c0, c1, l0, l1}
    StepArgs st;
    int32_t nchunks;
    int32_t max_cnt;
    uint32_t csr_bytes;        // bytes of the CSR-aligned arrays (S_old, S_new, Tfull of a one-rank run: 2m doubles) -- num_records of their buffer descriptors
    uint32_t t_bytes;          // bytes of Tfull (sharded runs: this rank's part of the reduce-scattered sums)
    uint32_t slice_bytes;      // bytes of s_slice (sharded runs)
    uint32_t seg_count;        // segments in cum / einfo / xt (device order, all ranks): cum has seg_count + 1 entries
    double fx_inv;             // 2^-fx_bits: Tfull holds fixed-point integers (fx_to_double)
};


// Sum the block partials in a fixed order, record the traces and run the early-stop
// rule of DESC_PGD.m:243-256 for the iteration whose objective just became known.
// t = 1-based index of the sweep that produced the partials.  Called by one full wave.
struct FinArgs {
    const double* partials; DevState* st; double* obj_trace; double* avg_trace;
    int64_t m; double stop_tol; int32_t nparts, t, patience, last_only;      // t == 0: nothing to do
    int64_t rank_stride; int32_t nranks;     // sharded runs: the partials of rank r start at partials + r * rank_stride (0 / 0: one rank)
};
// The sum of the workgroup partials is defined over 256 VIRTUAL lanes: virtual lane v adds the (rank, index) pairs v, v + 256, ... in that order, the
// 64 virtual lanes of a quarter are combined by the fixed DPP butterfly and the four quarters are added in index order.  A 256-thread block
// (finalize_block: the bookkeeping workgroup of the column-sum and unpack launches) gives a quarter to each of its waves; a single wave
// (finalize_wave: k_finalize) walks the four quarters one after the other -- the SAME bits either way, and the same on every rank.  Eight pairs are
// loaded before any is added (one at a time the 8 x 1024 pairs of a world-8 run were 128 dependent round trips for one wave: ~50 of the 85 us of
// k_unpack_S, profiles/r04_shard_w8_c4_rocprof.txt -- 35 us in the launches that book-keep nothing).
__device__ __forceinline__ void finalize_quarter(const FinArgs& f, int quarter, int lane, double& o, double& ch) {
    o = 0.0; ch = 0.0;
    const int E = max(f.nranks, 1) * f.nparts;
    for (int base = 64 * quarter + lane; base < E; base += 256 * 8) {
        double vo[8], vc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = base + 256 * u;
            vo[u] = 0.0; vc[u] = 0.0;
            if (idx < E) {
                const double* q = f.partials + (int64_t)(idx / f.nparts) * f.rank_stride + 2 * (int64_t)(idx % f.nparts);
                vo[u] = q[0]; vc[u] = q[1];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) { o += vo[u]; ch += vc[u]; }
    }
    o = group_sum<64>(o); ch = group_sum<64>(ch);
}
__device__ __forceinline__ void finalize_book(const FinArgs& f, double o, double ch);
// called by all 256 threads of a block
__device__ __forceinline__ void finalize_block(const FinArgs f) {
    __shared__ double s_fin[4][2];
    if (f.t <= 0 || f.st->stop) return;          // t == 0: no sweep to book-keep (uniform over the block)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double o, ch;
    finalize_quarter(f, wv, lane, o, ch);
    if (lane == 0) { s_fin[wv][0] = o; s_fin[wv][1] = ch; }
    __syncthreads();
    if (threadIdx.x == 0)
        finalize_book(f, ((s_fin[0][0] + s_fin[1][0]) + s_fin[2][0]) + s_fin[3][0], ((s_fin[0][1] + s_fin[1][1]) + s_fin[2][1]) + s_fin[3][1]);
}
// called by one full wave
__device__ __forceinline__ void finalize_wave(const FinArgs f) {
    if (f.t <= 0 || f.st->stop) return;
    const int lane = threadIdx.x & 63;
    double q0[4], q1[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) finalize_quarter(f, w, lane, q0[w], q1[w]);
    if (lane == 0) finalize_book(f, ((q0[0] + q0[1]) + q0[2]) + q0[3], ((q1[0] + q1[1]) + q1[2]) + q1[3]);
}
// traces and the stop rule of DESC_PGD.m:232-257 for the iteration whose sums just became known (one thread)
__device__ __forceinline__ void finalize_book(const FinArgs& f, double o, double ch) {
    DevState* st = f.st;
    // last_only: the partials come from the objective kernel after the final sweep t and
    // hold obj(t).  Otherwise they come from sweep t: obj(t-1) and sum|dS| of sweep t.
    const int t = f.t;
    const int it = f.last_only ? t : t - 1;          // iteration whose objective is o
    if (!f.last_only) f.avg_trace[t - 1] = ch / (double)f.m;                            // :232
    if (it >= 1) {
        f.obj_trace[it - 1] = o;                                                        // :233
        if (it <= st->last_tested) return;          // already tested (objective evaluated early by a download)
        st->last_tested = it;
        if (it > 1 && f.obj_trace[it - 2] - f.obj_trace[it - 1] < f.stop_tol) {         // :243
            st->misses += 1;
            if (st->misses >= f.patience) {                                             // :245-246
                st->stop = 1; st->iters_run = it; st->final_parity = it & 1;
            }
        } else {
            st->misses = 0;                                                             // :255
        }
    }
}

}  // namespace desc

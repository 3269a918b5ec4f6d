// Device-side text that more than one kernel unit of the PGD solver needs (pgd.hip, sweep_gather.hip, sweep_node.hip, sweep_band.hip):
// plain structs and __device__ __forceinline__ helpers only -- every __global__ kernel lives in exactly one .hip.
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

}  // namespace desc

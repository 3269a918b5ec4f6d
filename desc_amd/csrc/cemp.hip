// CEMP: cycle-edge message passing, Algorithms/CEMP.m:24-132.
//   :44-65   nsample 3-cycles per edge-with-cycles, sampled WITH replacement
//   :70-103  S0Mat(s,l) = |acos((tr(Rij Rjk Rki)-1)/2)|/pi, SVec = column means, 1 without cycles
//   :107-128 T rounds: w = exp(-beta (s_ik + s_jk)), column-normalised, s_ij = sum w .* S0
// The reference signs IndMat (CEMP.m:75-76) but only ever uses abs() of it; orientation
// matters solely for fetching R_jk / R_ki (stored block or its transpose).
// Same sweep shape as the PGD hot path with a fixed number of cycles per edge: one wave per
// edge (nsample <= 64 lanes; longer samples loop), two gathers of S per cycle, two wave
// reductions.
// Round 4: the rounds run on a CSR-ALIGNED copy of SVec (every edge value in both endpoint rows, as the PGD path's Sfull) in 2-D tiles
// (band of i-rows) x (block of j): the band's rows of S sit in the LDS (S({k,i}) = an LDS read), the rows of the j-block stay in the L2s
// because the grid walks the tiles j-block-major (S({j,k}) = a gather inside row j), and a tile's edges -- Ind is sorted by (i, j) -- are
// contiguous runs of the per-cycle arrays.  No host-side plan: a tile finds its edges by two binary searches per row.  Per cycle and round:
// 12 B streamed (packed row positions + S0) instead of 16 B + two random 8-byte gathers over the 20 MB of SVec (C4: 1.82 ms per round).
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "device_utils.h"
#include "cemp_math.h"
#include "cemp_state.h"

namespace desc {
namespace {

__global__ __launch_bounds__(256) void k_cemp_s0(const int32_t* pos_edge, const int32_t* ind_i, const int32_t* ind_j, const int32_t* kk,
                                                 const int32_t* e_jk, const int32_t* e_ki, const double* rij, double* S0,
                                                 double* S_a, double* S_b, int m_pos, int nsample, const int32_t* slot_a, const int32_t* slot_b) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t l = wid; l < m_pos; l += nw) {
        const int e = pos_edge[l], i = ind_i[e], j = ind_j[e];
        double A[9];
        load_block9(rij + 9 * (int64_t)e, A);
        double acc = 0.0;
        for (int s = lane; s < nsample; s += 64) {
            const int64_t c = l * nsample + s;
            const int k = kk[c];
            double pb[9], pc[9];                           // the two gathered blocks, in registers (16-byte loads)
            load_block9(rij + 9 * (int64_t)e_jk[c], pb);
            load_block9(rij + 9 * (int64_t)e_ki[c], pc);
            const double d = cemp_cycle_dist(A, pb, pc, !(j < k), !(k < i));
            S0[c] = d;
            acc += d;
        }
        acc = group_sum<64>(acc);
        if (lane == 0) {                                                                                     // :102
            const double mean = acc / (double)nsample;
            if (slot_a) { const int sa = slot_a[e], sb = slot_b[e]; S_a[sa] = mean; S_a[sb] = mean; S_b[sa] = mean; S_b[sb] = mean; }      // CSR-aligned copies
            else { S_a[e] = mean; S_b[e] = mean; }
        }
    }
}

// The same with the rotation blocks of node i's row staged in the LDS (round 4; CSR-aligned path: `pk` holds the position of k in row i): one
// 512-thread workgroup per node i, its edges (i, j) -- consecutive in the (i, j)-sorted list: node_seg[i] .. node_seg[i + 1] -- a wave each, R_ki of
// every sample an LDS read (80 B per slot for 16-byte reads); R_jk stays a gather from the edge table.  Same arithmetic in the same order.
__global__ __launch_bounds__(512) void k_cemp_s0_staged(const int32_t* pos_edge, const int32_t* ind_i, const int32_t* ind_j, const int32_t* kk, const int32_t* e_jk,
                                                        const uint32_t* pk, const int32_t* rowptr, const int32_t* adj_eid, const int32_t* node_seg, const double* rij, double* S0,
                                                        double* S_a, double* S_b, int n, int nsample, const int32_t* slot_a, const int32_t* slot_b) {
    extern __shared__ double s_blk[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int l0 = node_seg[i], l1 = node_seg[i + 1];
        if (l0 == l1) continue;
        const int r0 = rowptr[i], d = rowptr[i + 1] - r0;
        __syncthreads();
        for (int t = threadIdx.x; t < d; t += 512) {
            double Bk[9];
            load_block9(rij + 9 * (int64_t)adj_eid[r0 + t], Bk);
            for (int q = 0; q < 9; ++q) s_blk[10 * t + q] = Bk[q];
        }
        __syncthreads();
        for (int64_t l = l0 + wv; l < l1; l += 8) {
            const int e = pos_edge[l], j = ind_j[e];
            double A[9];
            load_block9(rij + 9 * (int64_t)e, A);
            double acc = 0.0;
            for (int s = lane; s < nsample; s += 64) {
                const int64_t c = l * nsample + s;
                const int k = kk[c];
                double pb[9], pc[9];
                load_block9(rij + 9 * (int64_t)e_jk[c], pb);
                const double* sb = s_blk + 10 * (int)(pk[c] & 0xFFFFu);
                const double2 c0 = *reinterpret_cast<const double2*>(sb), c1 = *reinterpret_cast<const double2*>(sb + 2), c2 = *reinterpret_cast<const double2*>(sb + 4),
                              c3 = *reinterpret_cast<const double2*>(sb + 6);
                pc[0] = c0.x; pc[1] = c0.y; pc[2] = c1.x; pc[3] = c1.y; pc[4] = c2.x; pc[5] = c2.y; pc[6] = c3.x; pc[7] = c3.y; pc[8] = sb[8];
                const double dd = cemp_cycle_dist(A, pb, pc, !(j < k), !(k < i));
                S0[c] = dd;
                acc += dd;
            }
            acc = group_sum<64>(acc);
            if (lane == 0) {                                                                                 // :102
                const double mean = acc / (double)nsample;
                const int sa = slot_a[e], sb2 = slot_b[e];
                S_a[sa] = mean; S_a[sb2] = mean; S_b[sa] = mean; S_b[sb2] = mean;
            }
        }
    }
}
// first natural segment (edge with cycles, ascending edge id) whose smaller endpoint is >= v; node_seg[n] = m_pos
__global__ __launch_bounds__(256) void k_cemp_node_seg(const int32_t* pos_edge, const int32_t* ind_i, int64_t m_pos, int n, int32_t* node_seg) {
    for (int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x; l < m_pos; l += (int64_t)gridDim.x * 256) {
        const int i = ind_i[pos_edge[l]], prev = l > 0 ? ind_i[pos_edge[l - 1]] : -1;
        for (int v = prev + 1; v <= i; ++v) node_seg[v] = (int32_t)l;
        if (l == m_pos - 1) for (int v = i + 1; v <= n; ++v) node_seg[v] = (int32_t)m_pos;
    }
}

// Epilogue MP = false: CEMP.m:125-126, the round's new s_ij.  MP = true: the H step of MPLS (MPLS.m:223-240) -- the gathered values are the
// residuals (S_old = ResVec), and the edge's h_ij goes straight into RH[e] = (1 - alpha) Res[e] + alpha h_ij (:240).
template <bool MP>
__device__ __forceinline__ void cemp_store(double* S_new, int slot_a, int slot_b, int e, double acc, const double* res, double* rh, double alpha) {
    if (MP) rh[e] = (1.0 - alpha) * res[e] + alpha * acc;
    else { S_new[slot_a] = acc; if (slot_b >= 0) S_new[slot_b] = acc; }
}

template <bool MP>
__global__ __launch_bounds__(256) void k_cemp_round(const int32_t* pos_edge, const int32_t* e_jk, const int32_t* e_ki, const double* S0,
                                                    const double* S_old, double* S_new, int m_pos, int nsample, double beta,
                                                    const double* res, double* rh, double alpha) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t l = wid; l < m_pos; l += nw) {
        const double acc = cemp_edge_round(l, lane, nsample, beta, e_jk, e_ki, S0, S_old);      // cemp_math.h
        if (lane == 0) cemp_store<MP>(S_new, pos_edge[l], -1, pos_edge[l], acc, res, rh, alpha);
    }
}

// slots of every edge in its two endpoint rows of the CSR-aligned arrays
__global__ __launch_bounds__(256) void k_cemp_slots(const int32_t* ind_i, const int32_t* ind_j, const int32_t* rowptr, const int32_t* adj, int32_t* slot_a, int32_t* slot_b, int64_t m) {
    auto slot = [&](int v, int u) {
        const int r = rowptr[v]; int lo = 0, hi = rowptr[v + 1] - r;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (adj[r + mid] < u) lo = mid + 1; else hi = mid; }
        return r + lo;
    };
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256) { slot_a[e] = slot(ind_i[e], ind_j[e]); slot_b[e] = slot(ind_j[e], ind_i[e]); }
}
__global__ __launch_bounds__(256) void k_cemp_extract(const double* Sfull, const int32_t* slot_a, double* S_vec, int64_t m) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m; e += (int64_t)gridDim.x * 256) S_vec[e] = Sfull[slot_a[e]];
}

// One round (CEMP.m:107-128) on the CSR-aligned copy, one workgroup per tile (band of BI consecutive nodes i) x (block of JB consecutive j); tiles are
// numbered j-block-major, so the workgroups in flight at any moment gather S({j,k}) from the same JB rows.  poe: edge -> index among the edges
// with cycles (NULL: every edge has cycles and the map is the identity).
constexpr int CEMP_MAXB = 16;                      // nodes per band at most
template <bool MP>
__global__ __launch_bounds__(256) void k_cemp_round_tile(const int32_t* rowptr, const int32_t* adj, const int32_t* adj_eid, const int32_t* poe, const int32_t* slot_b,
                                                         const uint32_t* pk, const double* S0, const double* S_old, double* S_new, int n, int BI, int JB, int n_iband,
                                                         int nsample, double beta, const double* res, double* rh, double alpha) {
    extern __shared__ double s_rows[];             // rows of the band: S_old[rowptr[i0] .. rowptr[i1])
    __shared__ int s_a[CEMP_MAXB], s_cnt[CEMP_MAXB + 1], s_rb[CEMP_MAXB];      // per node of the band: first slot of its run, edges in the tile, its row's offset in s_rows
    const int jb = blockIdx.x / n_iband, ib = blockIdx.x % n_iband;
    const int i0 = ib * BI, i1 = min(n, i0 + BI);
    const int j_lo = jb * JB, j_hi = min(n, j_lo + JB);
    if (j_hi <= i0 + 1) return;                    // every j of the block is <= every i of the band: no edge (i, j), i < j
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row_lo = rowptr[i0], row_len = rowptr[i1] - row_lo;
    if (tid < i1 - i0) {                           // the band's edges with j in the block: a contiguous run of row i's slots
        const int i = i0 + tid, r0 = rowptr[i], d = rowptr[i + 1] - r0;
        auto below = [&](int x) { int lo = 0, hi = d; while (lo < hi) { const int mid = (lo + hi) >> 1; if (adj[r0 + mid] < x) lo = mid + 1; else hi = mid; } return lo; };
        const int a = below(max(j_lo, i + 1)), b = below(j_hi);
        s_rb[tid] = r0 - row_lo;
        s_a[tid] = r0 + a; s_cnt[tid] = max(b - a, 0);        // a node of the band beyond the block's last j: no edge (b < a)
    }
    __syncthreads();
    int total = 0;
    for (int t = 0; t < i1 - i0; ++t) total += s_cnt[t];
    if (total == 0) return;
    for (int t = tid; t < row_len; t += 256) s_rows[t] = S_old[row_lo + t];
    __syncthreads();
    if (nsample <= 64) {
        // one sample per lane: CEMP_U edges of the tile per wave and trip, every stage's loads of all of them issued before any is used (each edge is
        // a chain of four dependent memory round trips -- slot -> row start of j and the packed word -> the gather in row j -> ... --: one edge at a
        // time the round measured 1.46 ms at C4, profiles/r04_cemp_tiles.txt)
        constexpr int CEMP_U = 4;                  // 2 / 4 / 6 / 8 edges in flight: 0.98 / 0.97 / 0.98 / 1.04 ms (profiles/r04_cemp_scalar_setup.txt): the round is issue-bound
        for (int x0 = wv; x0 < total; x0 += 4 * CEMP_U) {
            int rbi[CEMP_U], slot[CEMP_U], ee[CEMP_U], jn[CEMP_U]; bool on[CEMP_U];
#pragma unroll
            for (int u = 0; u < CEMP_U; ++u) {
                const int x = x0 + 4 * u;
                on[u] = x < total;
                int t = 0, y = on[u] ? x : 0;
                while (y >= s_cnt[t]) { y -= s_cnt[t]; ++t; }
                // everything about the edge is the same in all 64 lanes: scalar registers and scalar loads from here on (round 1.12 -> 0.97 ms at C4)
                rbi[u] = __builtin_amdgcn_readfirstlane(s_rb[t]); slot[u] = __builtin_amdgcn_readfirstlane(s_a[t] + y);
                ee[u] = uniform_load(adj_eid, slot[u]); jn[u] = uniform_load(adj, slot[u]);
            }
            int ll[CEMP_U], rbj[CEMP_U]; uint32_t pw[CEMP_U]; double dd[CEMP_U];
#pragma unroll
            for (int u = 0; u < CEMP_U; ++u) {
                ll[u] = poe ? uniform_load(poe, ee[u]) : ee[u];
                if (ll[u] < 0) on[u] = false;                   // no cycles: SVec stays 1 (:103, :126)
                rbj[u] = uniform_load(rowptr, jn[u]);
            }
#pragma unroll
            for (int u = 0; u < CEMP_U; ++u) {
                const int64_t c = (int64_t)max(ll[u], 0) * nsample + min(lane, nsample - 1);
                pw[u] = pk[c]; dd[u] = S0[c];
            }
            double sj[CEMP_U];
#pragma unroll
            for (int u = 0; u < CEMP_U; ++u) sj[u] = S_old[rbj[u] + (int)(pw[u] >> 16)];
#pragma unroll
            for (int u = 0; u < CEMP_U; ++u) {
                const bool act = lane < nsample;
                const double si = s_rows[rbi[u] + (int)(pw[u] & 0xFFFFu)];
                const double w = act ? exp(-beta * (si + sj[u])) : 0.0;                                     // :118-120  s_ik + s_jk
                const double rws = 1.0 / group_sum<64>(w);      // one division per edge (the reference divides every weight: the same to 1 ulp)
                const double acc = group_sum<64>(act ? (w * rws) * dd[u] : 0.0);                            // :122-125
                if (lane == 0 && on[u]) cemp_store<MP>(S_new, slot[u], MP ? -1 : slot_b[ee[u]], ee[u], acc, res, rh, alpha);
            }
        }
        return;
    }
    for (int x = wv; x < total; x += 4) {          // one wave per edge of the tile
        int t = 0, y = x;
        while (y >= s_cnt[t]) { y -= s_cnt[t]; ++t; }
        const int i = i0 + t, slot = s_a[t] + y;   // the edge (i, j): slot of j in row i
        const int e = adj_eid[slot], j = adj[slot];
        const int l = poe ? poe[e] : e;
        if (l < 0) continue;                       // no cycles: SVec stays 1 (:103, :126)
        const int rbi = rowptr[i] - row_lo, rbj = rowptr[j];
        double wr[4] = {0.0, 0.0, 0.0, 0.0}, dr[4] = {0.0, 0.0, 0.0, 0.0};
        double wsum = 0.0, acc = 0.0;
        if (nsample <= 4 * 64) {                   // weights stay in registers: one pass over the samples
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int sidx = lane + 64 * u;
                if (sidx < nsample) {
                    const int64_t c = (int64_t)l * nsample + sidx;
                    const uint32_t p = pk[c];
                    wr[u] = exp(-beta * (s_rows[rbi + (int)(p & 0xFFFFu)] + S_old[rbj + (int)(p >> 16)]));      // :118-120  s_ik + s_jk
                    dr[u] = S0[c];
                    wsum += wr[u];
                }
            }
            wsum = group_sum<64>(wsum);
            const double rws = 1.0 / wsum;
#pragma unroll
            for (int u = 0; u < 4; ++u) if (lane + 64 * u < nsample) acc += (wr[u] * rws) * dr[u];                 // :122-125
        } else {
            for (int sidx = lane; sidx < nsample; sidx += 64) {
                const uint32_t p = pk[(int64_t)l * nsample + sidx];
                wsum += exp(-beta * (s_rows[rbi + (int)(p & 0xFFFFu)] + S_old[rbj + (int)(p >> 16)]));
            }
            wsum = group_sum<64>(wsum);
            for (int sidx = lane; sidx < nsample; sidx += 64) {
                const int64_t c = (int64_t)l * nsample + sidx;
                const uint32_t p = pk[c];
                const double w = exp(-beta * (s_rows[rbi + (int)(p & 0xFFFFu)] + S_old[rbj + (int)(p >> 16)]));
                acc += (w / wsum) * S0[c];
            }
        }
        acc = group_sum<64>(acc);
        if (lane == 0) cemp_store<MP>(S_new, slot, MP ? -1 : slot_b[e], e, acc, res, rh, alpha);
    }
}

__global__ void k_fill1(double* p, int64_t n, double v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

__global__ __launch_bounds__(256) void k_cemp_inverse(const int32_t* pos_edge, int32_t* poe, int64_t m_pos) {
    for (int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x; l < m_pos; l += (int64_t)gridDim.x * 256) poe[pos_edge[l]] = (int32_t)l;
}
int env_int_c(const char* name, int dflt) { const char* v = std::getenv(name); return v ? std::atoi(v) : dflt; }

}  // namespace

int cemp_build(const desc_device_problem* dp, int32_t nsample, uint64_t seed, bool need_poe, CempState& st) {
    int rc = DESC_OK;
    const int64_t m = dp->m, n = dp->n;
    st.n = n; st.m = m; st.nsample = nsample;
    // samples: on the device; graphs beyond the device sampler's staging budget fall back to the host sampler
    int64_t mp = 0;
    int32_t max_deg = 0;
    const bool want_tiles = env_int_c("DESC_DEBUG_CEMP_TILES", 1) != 0;
    const bool by_rule = nsample <= 0;              // the caller left nsample to the sampler's rule (linprog_sij.m:43)
    rc = build_cemp_samples_device(dp, nsample, seed, &mp, &st.d_pos, &st.d_k, &st.d_ejk, &st.d_eki, want_tiles ? &st.d_pk : nullptr, &max_deg, &nsample);
    st.nsample = nsample;                           // by_rule: the value the sampler's rule gave
    for (void* q : {(void*)st.d_pos, (void*)st.d_k, (void*)st.d_ejk, (void*)st.d_eki, (void*)st.d_pk}) if (q) st.blocks.push_back(q);
    if (rc == DESC_ERR_TOO_LARGE) {
        if (by_rule) return rc;                     // the rule is the device sampler's: no host fall-back without an explicit nsample (the sampler
                                                    // hands the rule's value back before it refuses, so nsample itself no longer tells)
        hvec<int32_t> pos_edge, kk, e_jk, e_ki;
        const desc_problem hv = host_view(dp);
        if ((rc = build_cemp_samples_host(&hv, nsample, seed, pos_edge, kk, e_jk, e_ki))) return rc;
        mp = (int64_t)pos_edge.size();
        const int64_t mch = mp * nsample;
        if (mch >= (1ll << 31)) return fail(DESC_ERR_TOO_LARGE, "m_pos * nsample exceeds 2^31");
        if (mp) {
            if ((rc = st.alloc(&st.d_pos, mp)) || (rc = st.alloc(&st.d_k, mch)) || (rc = st.alloc(&st.d_ejk, mch)) || (rc = st.alloc(&st.d_eki, mch))) return rc;
            DESC_HIP(hipMemcpy(st.d_pos, pos_edge.data(), sizeof(int32_t) * mp, hipMemcpyHostToDevice));
            DESC_HIP(hipMemcpy(st.d_k, kk.data(), sizeof(int32_t) * mch, hipMemcpyHostToDevice));
            DESC_HIP(hipMemcpy(st.d_ejk, e_jk.data(), sizeof(int32_t) * mch, hipMemcpyHostToDevice));
            DESC_HIP(hipMemcpy(st.d_eki, e_ki.data(), sizeof(int32_t) * mch, hipMemcpyHostToDevice));
        }
    } else if (rc) return rc;
    const int64_t mc = mp * nsample;
    st.mp = mp; st.mc = mc; st.max_deg = max_deg;
    const int32_t *d_ii = dp->d_ii, *d_jj = dp->d_jj; const double* d_rij = dp->d_rij;
    // tiles: the device sampler delivered the packed row positions (rows shorter than 2^16); the band of one tile must fit the LDS
    const bool tiles = st.d_pk != nullptr && mp > 0 && max_deg > 0 && (size_t)max_deg * sizeof(double) <= 64 * 1024;
    st.tiles = tiles;
    const int64_t slen = tiles ? 2 * m : m;                                          // CSR-aligned: every edge value in both endpoint rows
    if ((rc = st.alloc(&st.d_S0, mc)) || (rc = st.alloc(&st.d_S[0], slen)) || (rc = st.alloc(&st.d_S[1], slen))) return rc;
    if (tiles && ((rc = st.alloc(&st.d_slot_a, m)) || (rc = st.alloc(&st.d_slot_b, m)) || (rc = st.alloc(&st.d_out, m)))) return rc;
    if (m) {
        const int g = (int)std::min<int64_t>(1024, (slen + 255) / 256);
        hipLaunchKernelGGL(k_fill1, dim3(g), dim3(256), 0, 0, st.d_S[0], slen, 1.0);     // SVec(~IndPosbin) = 1 (:103)
        hipLaunchKernelGGL(k_fill1, dim3(g), dim3(256), 0, 0, st.d_S[1], slen, 1.0);
        if (tiles) hipLaunchKernelGGL(k_cemp_slots, dim3((unsigned)std::min<int64_t>(4096, (m + 255) / 256)), dim3(256), 0, 0, d_ii, d_jj, dp->d_rowptr, dp->d_adj, st.d_slot_a, st.d_slot_b, m);
    }
    st.cur = 0;
    if (need_poe && mp == 0 && m) {                                                  // no edge has a cycle
        if ((rc = st.alloc(&st.d_poe, m))) return rc;
        DESC_HIP(hipMemsetAsync(st.d_poe, 0xFF, sizeof(int32_t) * m, 0));
    }
    if (!mp) return DESC_OK;
    st.g = (int)std::min<int64_t>(8192, (mp + 3) / 4);
    const size_t lds0 = (size_t)max_deg * 10 * sizeof(double);
    if (tiles && lds0 <= 150 * 1024 && env_int_c("DESC_DEBUG_STAGED_LAYOUT", 1) != 0) {       // node i's rotation blocks in the LDS
        int32_t* d_node_seg = nullptr;
        if ((rc = st.alloc(&d_node_seg, n + 1))) return rc;
        hipLaunchKernelGGL(k_cemp_node_seg, dim3((unsigned)std::min<int64_t>(4096, (mp + 255) / 256)), dim3(256), 0, 0, st.d_pos, d_ii, mp, (int)n, d_node_seg);
        if (lds0 > 64 * 1024) DESC_HIP(hipFuncSetAttribute((const void*)k_cemp_s0_staged, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds0));
        hipLaunchKernelGGL(k_cemp_s0_staged, dim3((unsigned)std::max<int64_t>(1, n)), dim3(512), lds0, 0, st.d_pos, d_ii, d_jj, st.d_k, st.d_ejk, st.d_pk, dp->d_rowptr, dp->d_adj_eid,
                           d_node_seg, d_rij, st.d_S0, st.d_S[0], st.d_S[1], (int)n, nsample, st.d_slot_a, st.d_slot_b);
    } else
    hipLaunchKernelGGL(k_cemp_s0, dim3(st.g), dim3(256), 0, 0, st.d_pos, d_ii, d_jj, st.d_k, st.d_ejk, st.d_eki, d_rij, st.d_S0, st.d_S[0], st.d_S[1], (int)mp, nsample,
                       tiles ? st.d_slot_a : (const int32_t*)nullptr, tiles ? st.d_slot_b : (const int32_t*)nullptr);
    // tile shape: the band's rows in <= 32 KiB of LDS (several workgroups per CU), the rows of a j-block ~2.5 MiB (they share an XCD's L2 with the streams)
    const int64_t avg_deg = std::max<int64_t>(1, 2 * m / std::max<int64_t>(1, n));
    int BI = (int)std::max<int64_t>(1, std::min<int64_t>(CEMP_MAXB, (32 * 1024 / 8) / std::max(max_deg, 1)));
    BI = std::max(1, std::min(BI, env_int_c("DESC_DEBUG_CEMP_BI", BI)));
    const int JB = (int)std::max<int64_t>(32, env_int_c("DESC_DEBUG_CEMP_JB", (int)std::max<int64_t>(32, (5ll << 19) / (8 * avg_deg))));      // measured: flat from ~2.5 MiB of rows on (profiles/r04_cemp_tile_scan.txt)
    st.BI = BI; st.JB = JB;
    st.n_iband = (int)((n + BI - 1) / BI); st.n_jblock = (int)((n + JB - 1) / JB);
    st.lds = (size_t)BI * (size_t)max_deg * sizeof(double);
    if ((tiles || need_poe) && mp != m) {                                            // edge -> index among the edges with cycles
        if ((rc = st.alloc(&st.d_poe, m))) return rc;
        DESC_HIP(hipMemsetAsync(st.d_poe, 0xFF, sizeof(int32_t) * m, 0));
        hipLaunchKernelGGL(k_cemp_inverse, dim3((unsigned)std::min<int64_t>(4096, (mp + 255) / 256)), dim3(256), 0, 0, st.d_pos, st.d_poe, mp);
    }
    if (tiles && st.lds > 64 * 1024) {
        DESC_HIP(hipFuncSetAttribute((const void*)k_cemp_round_tile<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)st.lds));
        DESC_HIP(hipFuncSetAttribute((const void*)k_cemp_round_tile<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)st.lds));
    }
    return DESC_OK;
}

int cemp_rounds(const desc_device_problem* dp, CempState& st, const double* beta, int32_t n_beta, int32_t max_iter, bool verbose) {
    if (!st.mp) {
        if (verbose) for (int it = 0; it < max_iter; ++it) printf("Reweighting Iteration %d Completed!\n", it + 1);
        return DESC_OK;
    }
    for (int it = 0; it < max_iter; ++it) {                                         // :107
        const double b = beta[it < n_beta ? it : n_beta - 1];                       // :30-34: missing betas repeat the last one
        const int cur = st.cur;
        if (st.tiles)
            hipLaunchKernelGGL(k_cemp_round_tile<false>, dim3((unsigned)((int64_t)st.n_iband * st.n_jblock)), dim3(256), st.lds, 0, dp->d_rowptr, dp->d_adj, dp->d_adj_eid, st.d_poe,
                               st.d_slot_b, st.d_pk, st.d_S0, st.d_S[cur], st.d_S[cur ^ 1], (int)st.n, st.BI, st.JB, st.n_iband, st.nsample, b,
                               (const double*)nullptr, (double*)nullptr, 0.0);
        else
            hipLaunchKernelGGL(k_cemp_round<false>, dim3(st.g), dim3(256), 0, 0, st.d_pos, st.d_ejk, st.d_eki, st.d_S0, st.d_S[cur], st.d_S[cur ^ 1], (int)st.mp, st.nsample, b,
                               (const double*)nullptr, (double*)nullptr, 0.0);
        st.cur ^= 1;
        if (verbose) printf("Reweighting Iteration %d Completed!\n", it + 1);   // MPLS.m:156
    }
    DESC_HIP(hipGetLastError());
    return DESC_OK;
}

const double* cemp_svec(CempState& st) {
    if (!st.tiles) return st.d_S[st.cur];
    hipLaunchKernelGGL(k_cemp_extract, dim3((unsigned)std::min<int64_t>(2048, (st.m + 255) / 256)), dim3(256), 0, 0, st.d_S[st.cur], st.d_slot_a, st.d_out, st.m);
    return st.d_out;
}

void cemp_hstep(const desc_device_problem* dp, CempState& st, const double* res_full, const double* res, double* rh, double beta, double alpha) {
    if (!st.mp) return;
    if (st.tiles)
        hipLaunchKernelGGL(k_cemp_round_tile<true>, dim3((unsigned)((int64_t)st.n_iband * st.n_jblock)), dim3(256), st.lds, 0, dp->d_rowptr, dp->d_adj, dp->d_adj_eid, st.d_poe,
                           st.d_slot_b, st.d_pk, st.d_S0, res_full, (double*)nullptr, (int)st.n, st.BI, st.JB, st.n_iband, st.nsample, beta, res, rh, alpha);
    else
        hipLaunchKernelGGL(k_cemp_round<true>, dim3(st.g), dim3(256), 0, 0, st.d_pos, st.d_ejk, st.d_eki, st.d_S0, res, (double*)nullptr, (int)st.mp, st.nsample, beta,
                           res, rh, alpha);
}

}  // namespace desc

using namespace desc;

extern "C" int desc_cemp_run(const desc_problem* prob, const double* beta, int32_t n_beta, int32_t max_iter, int32_t nsample,
                             uint64_t seed, int32_t device, double* s_vec, double* ms_total) {
    if (!prob || !s_vec || !beta) return fail(DESC_ERR_INVALID, "NULL argument");
    auto t0 = std::chrono::steady_clock::now();
    const int rc = with_uploaded(prob, device, [&](const desc_device_problem* dp) { return desc_cemp_run_dev(dp, beta, n_beta, max_iter, nsample, seed, s_vec, nullptr); });
    if (ms_total) *ms_total = ms_since(t0);
    return rc;
}

extern "C" int desc_cemp_run_dev(const desc_device_problem* dp, const double* beta, int32_t n_beta, int32_t max_iter, int32_t nsample,
                                 uint64_t seed, double* s_vec, double* ms_total) {
    return no_throw("desc_cemp_run_dev", [&]() -> int {
    if (!dp || !s_vec || !beta) return fail(DESC_ERR_INVALID, "NULL argument");
    if (n_beta < 1 || max_iter < 0 || nsample < 1) return fail(DESC_ERR_INVALID, "need n_beta >= 1, max_iter >= 0, nsample >= 1");
    int rc = DESC_OK;
    auto t0 = std::chrono::steady_clock::now();
    DESC_HIP(hipSetDevice(dp->device));
    CempState st;
    if ((rc = cemp_build(dp, nsample, seed, false, st))) return rc;                  // CEMP.m:44-103
    if ((rc = cemp_rounds(dp, st, beta, n_beta, max_iter, false))) return rc;        // :107-128
    const double* d_svec = dp->m ? cemp_svec(st) : nullptr;
    DESC_HIP(hipDeviceSynchronize());
    if (dp->m) DESC_HIP(hipMemcpy(s_vec, d_svec, sizeof(double) * dp->m, hipMemcpyDeviceToHost));
    if (ms_total) *ms_total = ms_since(t0);
    return DESC_OK;
    });
}

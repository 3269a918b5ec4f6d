// Set-up of the node layout of the DESC projected-gradient solver on gfx950: the kernels that build it and setup_node, which plans and launches them.
//
// Two layouts of the same arithmetic, three sweep kernels (SWEEP VARIANTS):
//
//  NODE layout (default).  Edges with cycles are stored band-major: nodes are cut into bands
//  of B consecutive ids and the edges (i,j) of a band are ordered by (j,i), so that a
//  run of consecutive segments shares j (its row of S stays in the CU's L1) while the
//  band's i-rows stay in the XCD's L2.  S_vec is kept CSR-aligned (`Sfull`, every edge
//  value stored in both endpoint rows) so S({j,k}) = Sfull[rowptr[j] + idx_j(k)] is a
//  gather inside one contiguous row.  Per cycle one packed word holds idx_i(k), idx_j(k)
//  and the two mirror-present bits (DESC_PGD.m:113,124).  The mirror sums are column
//  sums of per-node weight matrices (k_colsum_node, pgd.hip).
//    HBM traffic per cycle and iteration: sweep 28 B (w r/w 16, S0 8, packed word 4)
//    + column sums (w 8 + a 2-byte column index for the mirrored cycles only), plus the row
//    gathers of S served by L1/L2.
//    Two sweeps run on this layout.  k_sweep_band (default since round 2, segments <= 256 cycles): bands sized so that their
//    CSR rows fit the LDS of a CU, one workgroup per CU (8 waves; shapes: band_shape()), S({k,i}) from the LDS,
//    register-pipelined waves, work dealt in j-block-major units so that the rows of S({j,k}) stay in the L2s; the Adam plugin on
//    its own instances up to 64 cycles.  k_sweep_node (round 1; tiny graphs, rows beyond the LDS, Adam on longer segments):
//    L2-sized bands, 512-thread workgroups, chunks staged through the LDS.
//
//  GATHER (fallback: max degree >= 32768, more LDS than a workgroup may hold, or
//  segments longer than 256 cycles).  Natural edge order; per cycle e_jk, e_ki, ikj, jki
//  and element-granular gathers S[e_jk], S[e_ki], w[ikj], w[jki]  (72 B per cycle as
//  SURVEY.md 8d counts them).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "pgd_handle.h"

namespace desc {

// the same with the third factor already loaded (k_layout_node_dev<.., STAGED>: node i's blocks sit in the LDS)
__device__ __forceinline__ double cycle_trace_regs(const double* A, const double* pb, bool tb, const double* Cm, bool tc) {
    double Bm[9], B[9], C[9];
    load_block9(pb, Bm);
    for (int r = 0; r < 3; ++r)
        for (int s = 0; s < 3; ++s) {
            B[r + 3 * s] = tb ? Bm[s + 3 * r] : Bm[r + 3 * s];
            C[r + 3 * s] = tc ? Cm[s + 3 * r] : Cm[r + 3 * s];
        }
    double tr = 0.0;
    for (int r = 0; r < 3; ++r) {
        double P[3];
        for (int s = 0; s < 3; ++s) {
            double acc = 0.0;
            for (int u = 0; u < 3; ++u) acc = acc + A[r + 3 * u] * B[u + 3 * s];
            P[s] = acc;
        }
        double acc = 0.0;
        for (int u = 0; u < 3; ++u) acc = acc + P[u] * C[u + 3 * r];
        tr = tr + acc;
    }
    return tr;
}

// Setup of the node layout: packs idx_i(k) / idx_j(k) / mirror bits of every cycle and
// evaluates its inconsistency.  kf = k | (ikj>=0)<<30 | (jki>=0)<<31, already in device
// (band-major) order.
__global__ __launch_bounds__(256) void k_layout_node(const int32_t* cum, const int32_t* pos_edge,
                                                     const int32_t* ind_i, const int32_t* ind_j, const uint32_t* kf,
                                                     const int32_t* rowptr, const int32_t* adj, const int32_t* adj_eid,
                                                     const double* rij, uint32_t* pk, double* S0, int m_pos) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t l = wid; l < m_pos; l += nw) {
        const int base = cum[l], cnt = cum[l + 1] - base;
        const int e = pos_edge[l], i = ind_i[e], j = ind_j[e];
        const int ri = rowptr[i], di = rowptr[i + 1] - ri, rj = rowptr[j], dj = rowptr[j + 1] - rj;
        double A[9];
        for (int t = 0; t < 9; ++t) A[t] = rij[9 * (int64_t)e + t];
        for (int q = lane; q < cnt; q += 64) {
            const uint32_t x = kf[(int64_t)base + q];
            const int k = (int)(x & 0x3FFFFFFFu);
            int lo = 0, hi = di;                                  // idx_i(k): position of k in row i
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (adj[ri + mid] < k) lo = mid + 1; else hi = mid; }
            const int xi = min(lo, max(di - 1, 0));               // clamp: memory-safe even for a bogus imported structure
            lo = 0; hi = dj;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (adj[rj + mid] < k) lo = mid + 1; else hi = mid; }
            const int xj = min(lo, max(dj - 1, 0));
            pk[(int64_t)base + q] = (uint32_t)xi | ((x >> 30) & 1u) << 15 | (uint32_t)xj << 16 | ((x >> 31) & 1u) << 31;
            const double tr = cycle_trace(A, rij + 9 * (int64_t)adj_eid[rj + xj], !(j < k), rij + 9 * (int64_t)adj_eid[ri + xi], !(k < i));
            S0[(int64_t)base + q] = abs_acos_ext((tr - 1.0) / 2.0) / M_PI;
        }
    }
}

// The same for a device-built structure, in place: reads the sampled k (natural order), decides
// the two mirror-present bits from the selection thresholds of the partner edges -- cycle (ik;j)
// was sampled iff (key(e_ik, j), j) <= (tau, ktau) of edge {i,k} -- and does the within-segment
// re-ordering [(ik;j) only | both mirrors | (jk;i) only | none] in the wave (stable: ascending k
// inside a class, exactly like the host path).  Segments have <= MAX_SEG_CYCLES cycles (pieces of 64).
// STAGED (round 4; natural order only: the segments of a node are then consecutive, node_seg[i] .. node_seg[i + 1]): one workgroup per node i
// first copies the rotation blocks of ALL edges incident to i -- row i of the CSR, 72 B per slot, 80 B apart in the LDS for 16-byte reads -- so that
// R_ki of every cycle of every segment (i, .) is an LDS read; R_jk stays a gather from the edge table.  Half of the kernel's 2 x 72 B of gathers per
// cycle (125 M cycles at C4: 18 GB out of the caches) become 0.36 GB of staging.
template <int NP, bool STAGED>                       // NP: pieces of 64 cycles per segment: 1, 2 or 4; STAGED: 512 threads (8 waves share a node's blocks), else 256
__global__ __launch_bounds__(STAGED ? 512 : 256) void k_layout_node_dev(const int32_t* cum, const int32_t* src_start, const int32_t* pos_edge,
                                                         const int32_t* ind_i, const int32_t* ind_j, const int32_t* nat_k,
                                                         const unsigned long long* tau, const int32_t* ktau,
                                                         uint64_t seed, const int32_t* rowptr, const unsigned long long* bits,
                                                         const uint32_t* rank, int words, const int32_t* adj_eid, const double* rij,
                                                         uint32_t* pk, double* S0, uint8_t* seg_perm, uint32_t* seg_counts, int m_pos, const int32_t* node_seg, int n_nodes) {
    extern __shared__ double s_blk[];                // STAGED: 10 doubles per slot of row i (9 used)
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * 256) >> 6;
    const int n_outer = STAGED ? n_nodes : 1;
    for (int node = STAGED ? blockIdx.x : 0; node < n_outer; node += STAGED ? gridDim.x : 1) {
    int64_t l_first = wid, l_end = m_pos, l_step = nw;
    if (STAGED) {
        l_first = node_seg[node] + (threadIdx.x >> 6); l_end = node_seg[node + 1]; l_step = 8;
        if (node_seg[node] == l_end) continue;       // no segment with this smaller endpoint (uniform over the workgroup)
        const int r0n = rowptr[node], dn = rowptr[node + 1] - r0n;
        __syncthreads();                             // the previous node's blocks are no longer read
        for (int t = threadIdx.x; t < dn; t += 512) {
            double Bk[9];
            load_block9(rij + 9 * (int64_t)adj_eid[r0n + t], Bk);
            for (int q = 0; q < 9; ++q) s_blk[10 * t + q] = Bk[q];
        }
        __syncthreads();
    }
    for (int64_t l = l_first; l < l_end; l += l_step) {
        const int base = cum[l], cnt = cum[l + 1] - base, src = src_start[l];
        const int e = pos_edge[l], i = ind_i[e], j = ind_j[e];
        const int ri = rowptr[i], di = rowptr[i + 1] - ri, rj = rowptr[j], dj = rowptr[j + 1] - rj;
        double A[9];
        for (int t = 0; t < 9; ++t) A[t] = rij[9 * (int64_t)e + t];
        // pass 1: per cycle the packed word, the two partner edges and its class; class sizes per piece
        uint32_t word[NP]; int eik[NP], ejk[NP], kk[NP], cls[NP];
        unsigned long long cm[NP][4];
        int ncls[4] = {0, 0, 0, 0};
#pragma unroll
        for (int pc = 0; pc < NP; ++pc) {
            const int t = pc * 64 + lane;
            const bool on = t < cnt;
            int k = 0, xi = 0, xj = 0, ei2 = e, ej2 = e;
            bool fi = false, fj = false;
            if (on) {
                k = nat_k[(int64_t)src + t];
                // idx_i(k), idx_j(k): positions of k in rows i and j = rank of its bit in the adjacency bitmaps
                const size_t wi = (size_t)i * words + (k >> 6), wj = (size_t)j * words + (k >> 6);
                const unsigned long long below = (1ull << (k & 63)) - 1ull;
                xi = min((int)(rank[wi] + __popcll(bits[wi] & below)), max(di - 1, 0));
                xj = min((int)(rank[wj] + __popcll(bits[wj] & below)), max(dj - 1, 0));
                ei2 = adj_eid[ri + xi]; ej2 = adj_eid[rj + xj];
                {   // both partner edges lie on the triangle {i,j,k}: they have cycles, their thresholds are defined
                    const unsigned long long key = d_sample_key(seed, (uint64_t)ei2, (uint64_t)j), th = tau[ei2];
                    fi = key < th || (key == th && j <= ktau[ei2]);                            // IKJ_appears (:113)
                }
                {
                    const unsigned long long key = d_sample_key(seed, (uint64_t)ej2, (uint64_t)i), th = tau[ej2];
                    fj = key < th || (key == th && i <= ktau[ej2]);                            // JKI_appears (:124)
                }
            }
            word[pc] = (uint32_t)xi | (fi ? 1u : 0u) << 15 | (uint32_t)xj << 16 | (fj ? 1u : 0u) << 31;
            eik[pc] = ei2; ejk[pc] = ej2; kk[pc] = k;
            cls[pc] = !on ? 4 : fi ? (fj ? 1 : 0) : (fj ? 2 : 3);
#pragma unroll
            for (int c = 0; c < 4; ++c) { cm[pc][c] = __ballot(cls[pc] == c); ncls[c] += __popcll(cm[pc][c]); }
        }
        if (lane == 0) seg_counts[l] = (uint32_t)ncls[0] | (uint32_t)(ncls[0] + ncls[1]) << 9 | (uint32_t)ncls[2] << 18;
        // pass 2: stable placement (class, then natural order) and the cycle inconsistency
        const int cbase[4] = {0, ncls[0], ncls[0] + ncls[1], ncls[0] + ncls[1] + ncls[2]};
        const unsigned long long lt = (1ull << lane) - 1ull;
        int seen[4] = {0, 0, 0, 0};
#pragma unroll
        for (int pc = 0; pc < NP; ++pc) {
            if (pc * 64 >= cnt) break;                 // wave-uniform
            const int c = cls[pc];
            if (c < 4) {
                const int o = cbase[c] + seen[c] + __popcll(cm[pc][c] & lt);
                const int k = kk[pc];
                pk[(int64_t)base + o] = word[pc];
                seg_perm[(int64_t)base + o] = (uint8_t)(pc * 64 + lane);
                double tr;
                if (STAGED) {
                    double Cm[9];
                    const double* sb = s_blk + 10 * (int)(word[pc] & 0x7FFFu);          // slot idx_i(k) of row i: the block of edge {i, k}
                    const double2 c0 = *reinterpret_cast<const double2*>(sb), c1 = *reinterpret_cast<const double2*>(sb + 2), c2 = *reinterpret_cast<const double2*>(sb + 4),
                                  c3 = *reinterpret_cast<const double2*>(sb + 6);
                    Cm[0] = c0.x; Cm[1] = c0.y; Cm[2] = c1.x; Cm[3] = c1.y; Cm[4] = c2.x; Cm[5] = c2.y; Cm[6] = c3.x; Cm[7] = c3.y; Cm[8] = sb[8];
                    tr = cycle_trace_regs(A, rij + 9 * (int64_t)ejk[pc], !(j < k), Cm, !(k < i));
                } else tr = cycle_trace(A, rij + 9 * (int64_t)ejk[pc], !(j < k), rij + 9 * (int64_t)eik[pc], !(k < i));
                S0[(int64_t)base + o] = abs_acos_ext((tr - 1.0) / 2.0) / M_PI;
            }
#pragma unroll
            for (int c2 = 0; c2 < 4; ++c2) seen[c2] += __popcll(cm[pc][c2]);
        }
    }
    }
}
// node_seg[v] = first natural segment (edge with cycles, ascending edge id) whose smaller endpoint is >= v; node_seg[n] = m_pos.  Ind is sorted by
// (i, j): the thread at every change of i fills the gap of nodes without segments below it.
__global__ __launch_bounds__(256) void k_node_seg_start(const int32_t* pos_edge, const int32_t* ind_i, int64_t m_pos, int n, int32_t* node_seg) {
    for (int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x; l < m_pos; l += (int64_t)gridDim.x * 256) {
        const int i = ind_i[pos_edge[l]], prev = l > 0 ? ind_i[pos_edge[l - 1]] : -1;
        for (int v = prev + 1; v <= i; ++v) node_seg[v] = (int32_t)l;
        if (l == m_pos - 1) for (int v = i + 1; v <= n; ++v) node_seg[v] = (int32_t)m_pos;
    }
}
// Device-order segment tables from the plan's permutation (device-built structures): segment q of the device order is the
// structure's edge-with-cycles number order[q]
__global__ __launch_bounds__(256) void k_seg_tables(const int32_t* order, const int32_t* nat_pos_edge, const int32_t* nat_cum, int32_t* cum,
                                                    int32_t cyc_lo, int32_t* src_start, int32_t* pos_edge2, int32_t* devpos, int64_t m_pos) {
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q <= m_pos; q += (int64_t)gridDim.x * 256) {
        cum[q] -= cyc_lo;                                  // local cycle numbering (meaningful for owned segments)
        if (q == m_pos) break;
        const int32_t l = order[q], e = nat_pos_edge[l];
        src_start[q] = nat_cum[l];
        pos_edge2[q] = e; devpos[e] = (int32_t)q;
    }
}
// Round 4: a one-rank handle computes the packed words, S0_long and the in-segment class order in the structure's NATURAL order as soon as the
// sampled cycles exist -- while the host is still planning the band-major order (8-9 ms at C4) -- and moves whole segments to their device
// positions afterwards: segment q of the device order is natural segment order[q].  One wave per segment; ~26 bytes per cycle, bandwidth-bound.
__global__ __launch_bounds__(256) void k_permute_segments(const int32_t* order, const int32_t* nat_cum, const int32_t* cum, const uint32_t* pk_nat, const double* S0_nat,
                                                          const uint8_t* perm_nat, const uint32_t* counts_nat, uint32_t* pk, double* S0, uint8_t* seg_perm, uint32_t* counts,
                                                          int64_t m_pos) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * 256) >> 6;
    // PU segments in flight per wave: a segment alone is a chain of three dependent round trips (order -> starts -> data) for ~1 KB moved
    constexpr int PU = 4;
    for (int64_t q0 = wid * PU; q0 < m_pos; q0 += nw * PU) {
        int32_t l[PU]; int64_t src[PU], dst[PU]; int cnt[PU];
#pragma unroll
        for (int u = 0; u < PU; ++u) l[u] = order[min(q0 + u, m_pos - 1)];
#pragma unroll
        for (int u = 0; u < PU; ++u) {
            const int64_t q = min(q0 + u, m_pos - 1);
            src[u] = nat_cum[l[u]]; dst[u] = cum[q];
            cnt[u] = q0 + u < m_pos ? cum[q + 1] - cum[q] : 0;
        }
        uint32_t a[PU]; double b[PU]; uint8_t c[PU];
#pragma unroll
        for (int u = 0; u < PU; ++u)
            if (lane < cnt[u]) { a[u] = pk_nat[src[u] + lane]; b[u] = S0_nat[src[u] + lane]; c[u] = perm_nat[src[u] + lane]; }
#pragma unroll
        for (int u = 0; u < PU; ++u) {
            if (lane < cnt[u]) { pk[dst[u] + lane] = a[u]; S0[dst[u] + lane] = b[u]; seg_perm[dst[u] + lane] = c[u]; }
            for (int t = lane + 64; t < cnt[u]; t += 64) { pk[dst[u] + t] = pk_nat[src[u] + t]; S0[dst[u] + t] = S0_nat[src[u] + t]; seg_perm[dst[u] + t] = perm_nat[src[u] + t]; }
            if (lane == 0 && q0 + u < m_pos) counts[q0 + u] = counts_nat[l[u]];
        }
    }
}
// per-edge slots of the CSR-aligned arrays, on the device (device-built structures): eslot[e] = this
// edge's slot in its smaller endpoint's row; einfo of the edges with cycles in device order
__global__ __launch_bounds__(256) void k_edge_slots(const int32_t* ind_i, const int32_t* ind_j, const int32_t* rowptr, const int32_t* adj,
                                                    const int32_t* pos_edge2, int32_t* eslot, EdgeInfo* einfo, int64_t m, int64_t m_pos) {
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, nt = (int64_t)gridDim.x * 256;
    auto slot = [&](int v, int u) {                   // position of u in row v
        const int r = rowptr[v]; int lo = 0, hi = rowptr[v + 1] - r;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (adj[r + mid] < u) lo = mid + 1; else hi = mid; }
        return r + lo;
    };
    for (int64_t e = t0; e < m; e += nt) eslot[e] = slot(ind_i[e], ind_j[e]);
    for (int64_t q = t0; q < m_pos; q += nt) {
        const int e = pos_edge2[q], i = ind_i[e], j = ind_j[e];
        einfo[q] = EdgeInfo{rowptr[i], rowptr[j], slot(i, j), slot(j, i)};
    }
}
// Record of a CSR slot (v,u) for the column-sum pass: {first cycle of the run of segment {v,u} that contributes to node v's
// columns, length of the run | (v is the smaller endpoint) << 31}.  counts = n_ionly | n_i << 9 | n_jonly << 18 of the segment
// (class order [(ik;j) only | both | (jk;i) only | none]): the smaller endpoint reads [0, n_i), the larger [n_ionly, n_i + n_jonly).
__host__ __device__ inline int2 slot_record(int32_t seg_first, uint32_t counts, bool v_is_i) {
    const int n_io = counts & 0x1FFu, n_i = (counts >> 9) & 0x1FFu, n_jo = (counts >> 18) & 0x1FFu;
    return v_is_i ? int2{seg_first, (int)((uint32_t)n_i | 0x80000000u)} : int2{seg_first + n_io, n_i - n_io + n_jo};
}
// CSR-aligned segment records for the column-sum pass: 16 lanes per node row
__global__ __launch_bounds__(256) void k_adj_seg(const int32_t* rowptr, const int32_t* adj, const int32_t* adj_eid, const int32_t* devpos,
                                                 const int32_t* cum, const uint32_t* seg_counts, int seg_lo, int seg_hi, int2* adj_seg, int n) {
    const int l16 = threadIdx.x & 15;
    const int row0 = (blockIdx.x * 256 + threadIdx.x) >> 4, nrows = (gridDim.x * 256) >> 4;
    for (int v = row0; v < n; v += nrows)
        for (int t = rowptr[v] + l16; t < rowptr[v + 1]; t += 16) {
            const int q = devpos[adj_eid[t]];
            int2 rec{0, 0};
            if (q >= seg_lo && q < seg_hi) rec = slot_record(cum[q], seg_counts[q], v < adj[t]);
            adj_seg[t] = rec;
        }
}

// ---- the column-index stream of the column-sum pass
__device__ __forceinline__ int slot_nact(int2 rec) { return rec.y & 0x1FF; }         // contributing cycles of the segment behind a CSR slot, seen from the row's node
// entries per node row (16 lanes per row)
__global__ __launch_bounds__(256) void k_midx_rowsum(const int32_t* rowptr, const int2* adj_seg, uint32_t* rowsum, int n) {
    const int l16 = threadIdx.x & 15;
    const int row0 = (blockIdx.x * 256 + threadIdx.x) >> 4, nrows = (gridDim.x * 256) >> 4;
    for (int vb = row0 - (row0 % 4); vb < n; vb += nrows) {
        const int v = vb + (row0 % 4);
        int acc = 0;
        if (v < n) for (int t = rowptr[v] + l16; t < rowptr[v + 1]; t += 16) acc += slot_nact(adj_seg[t]);
        acc = group16_sum(acc);
        if (v < n && l16 == 0) rowsum[v] = (uint32_t)acc;
    }
}
// moff[t] = rowbase[v] + (entries of the earlier slots of row v).  16 lanes per row, each walking one contiguous sixteenth of
// the row's slots (offsets by a 16-lane exclusive scan of the chunk totals)
__global__ __launch_bounds__(256) void k_midx_fill(const int32_t* rowptr, const int2* adj_seg, const uint32_t* rowbase,
                                                   uint32_t* moff, int n) {
    const int l16 = threadIdx.x & 15;
    const int row0 = (blockIdx.x * 256 + threadIdx.x) >> 4, nrows = (gridDim.x * 256) >> 4;
    for (int vb = row0 - (row0 % 4); vb < n; vb += nrows) {      // the 4 rows of a wave advance together (full-wave shuffles)
        const int v = vb + (row0 % 4);
        int t0 = 0, t1 = 0;
        if (v < n) {
            const int r0 = rowptr[v], r1 = rowptr[v + 1], chunk = (r1 - r0 + 15) / 16;
            t0 = min(r0 + l16 * chunk, r1); t1 = min(t0 + chunk, r1);
        }
        int mine = 0;
        for (int t = t0; t < t1; ++t) mine += slot_nact(adj_seg[t]);
        int incl = mine;                                          // inclusive scan over the 16 lanes of the row
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) { const int up = __shfl_up(incl, d, 16); if (l16 >= d) incl += up; }
        if (v >= n) continue;
        uint32_t o = rowbase[v] + (uint32_t)(incl - mine);
        for (int t = t0; t < t1; ++t) { moff[t] = o; o += (uint32_t)slot_nact(adj_seg[t]); }
    }
}
// ... and the entries themselves: 16 lanes per CSR slot, lanes over the slot's contributing cycles (coalesced both ways)
__global__ __launch_bounds__(256) void k_midx_entries(const int2* adj_seg, const uint32_t* moff, const uint32_t* pk, uint16_t* midx, int64_t nslots) {
    const int l16 = threadIdx.x & 15;
    const int64_t g0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4, ng = ((int64_t)gridDim.x * 256) >> 4;
    for (int64_t t = g0; t < nslots; t += ng) {
        const int2 rec = adj_seg[t];
        const bool v_is_i = rec.y < 0;
        const int nact = slot_nact(rec);
        const uint32_t o = moff[t];
        for (int q = l16; q < nact; q += 16) {
            const uint32_t p = pk[(int64_t)rec.x + q];
            midx[(size_t)o + q] = (uint16_t)((v_is_i ? p : p >> 16) & 0x7FFFu);
        }
    }
}

// ---- exchange layout of the sharded runs (round 3) -------------------------------------------------------------------
// Rank r owns the nodes [node_lo[r], node_lo[r+1]) (whole bands) and with them the edges (i, j), i < j, whose SMALLER endpoint it owns:
// a contiguous range [e_lo[r], e_lo[r+1]) of the (i,j)-sorted edge list.  Its part of the reduce-scatter buffer (t_part = 2 t_half doubles):
//   [0, t_half)        T1 of its edges, in edge order            -> node i's column-sum workgroup writes the T1 of ALL its larger
//                                                                   neighbours as ONE contiguous run (CSR order of row i = edge order)
//   [t_half, 2 t_half) T2 of its edges, ordered by (j, i)        -> node j's workgroup writes its smaller neighbours' T2 as at most
//                                                                   `world` contiguous runs (the smaller neighbours owned by one rank
//                                                                   are consecutive in row j)
// (round 2 ordered both halves by the sweep's segment order (band, j, i): every rank wrote all 2m slots 8 bytes at a time, +58 us per
//  iteration at C4 whatever the number of ranks).  The all-gather slice of a rank = S of its edges in edge order, so the unpack copies
//  the larger-neighbour half of every CSR row contiguously and gathers the other half.
// prefB[r * n + v] = number of T2 entries of owner r that precede node v's run = sum over v' < v of |{u < v', u owned by r}|
__device__ __forceinline__ int nbrs_below(const int32_t* adj, int r0, int r1, int x) {       // neighbours of the row smaller than x
    int lo = 0, hi = r1 - r0;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (adj[r0 + mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}
__global__ __launch_bounds__(1024) void k_prefB(const int32_t* rowptr, const int32_t* adj, const int32_t* node_lo, int32_t* prefB, int n) {
    __shared__ int sa[1024];
    __shared__ int carry;
    const int r = blockIdx.x, vlo = node_lo[r], vhi = node_lo[r + 1];
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int v = base + threadIdx.x;
        int c = 0;
        if (v < n) { const int r0 = rowptr[v], r1 = rowptr[v + 1]; c = nbrs_below(adj, r0, r1, min(vhi, v)) - nbrs_below(adj, r0, r1, min(vlo, v)); }
        sa[threadIdx.x] = c;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int x = threadIdx.x >= d ? sa[threadIdx.x - d] : 0;
            __syncthreads();
            sa[threadIdx.x] += x;
            __syncthreads();
        }
        if (v < n) prefB[(int64_t)r * n + v] = carry + sa[threadIdx.x] - c;
        __syncthreads();
        if (threadIdx.x == 1023) carry += sa[1023];
        __syncthreads();
    }
}
// Sharded column sums: the run of row v's CSR slots whose segments {v, u} belong to the rank that owns the nodes [lo, hi) -- those with
// min(v, u) in [lo, hi): u >= lo when v itself is owned, lo <= u < hi when v >= hi, none when v < lo.  Neighbours are ascending: one run.
__global__ __launch_bounds__(256) void k_node_runs(const int32_t* rowptr, const int32_t* adj, int lo, int hi, int2* runs, int n) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int r0 = rowptr[v], r1 = rowptr[v + 1];
    int2 run{0, 0};
    if (v >= lo) {
        run.x = nbrs_below(adj, r0, r1, lo);
        run.y = v < hi ? r1 - r0 : nbrs_below(adj, r0, r1, hi);
    }
    runs[v] = run;
}
__device__ __forceinline__ int owner_of_node(const int32_t* node_lo, int world, int v) { int r = 0; while (r + 1 < world && v >= node_lo[r + 1]) ++r; return r; }
// Exchange parts (round 4): the owners of the layout are VIRTUAL -- vo = rank * xparts + part, node ranges node_lo[vo .. vo + 1), nv = world * xparts of
// them -- and the send buffer is part-major: block (part * world + rank) holds [T1 | T2] of that virtual owner's edges, so that the reduce-scatter of
// part c is ONE collective over the contiguous blocks [c * world, (c + 1) * world) and can travel while part c - 1 is swept.  xparts = 1: round 3's layout.
__device__ __forceinline__ int xblock_of(int vo, int xparts, int world) { return (vo % xparts) * world + vo / xparts; }
// xpos[t]: where the column sum of CSR slot t = (v, u) goes in the send buffer; spos[t]: where S of edge {v, u} sits in the gathered slices (per REAL rank)
__global__ __launch_bounds__(256) void k_xpos(const int32_t* rowptr, const int32_t* adj, const int32_t* adj_eid, const int32_t* node_lo, const int32_t* e_lo,
                                              const int32_t* prefB, int nv, int xparts, int world, int64_t t_part, int64_t slice_len, int32_t* xpos, int32_t* spos, int n) {
    const int l16 = threadIdx.x & 15;
    const int row0 = (blockIdx.x * 256 + threadIdx.x) >> 4, nrows = (gridDim.x * 256) >> 4;
    const int64_t t_half = t_part / 2;
    for (int v = row0; v < n; v += nrows) {
        const int r0 = rowptr[v], r1 = rowptr[v + 1];
        const int ov = owner_of_node(node_lo, nv, v);
        for (int t = r0 + l16; t < r1; t += 16) {
            const int u = adj[t], e = adj_eid[t];
            if (u > v) {                                         // T1 of edge (v, u); S of the edge: both with the owner of v
                xpos[t] = (int32_t)((int64_t)xblock_of(ov, xparts, world) * t_part + (e - e_lo[ov]));
                spos[t] = (int32_t)((int64_t)(ov / xparts) * slice_len + (e - e_lo[(ov / xparts) * xparts]));
            } else {                                             // column u of node v = T2 of edge (u, v), owned by the owner of u
                const int ou = owner_of_node(node_lo, nv, u);
                const int first = nbrs_below(adj, r0, r1, node_lo[ou]);          // first smaller neighbour of v that ou owns
                xpos[t] = (int32_t)((int64_t)xblock_of(ou, xparts, world) * t_part + t_half + prefB[(int64_t)ou * n + v] + ((t - r0) - first));
                spos[t] = (int32_t)((int64_t)(ou / xparts) * slice_len + (e - e_lo[(ou / xparts) * xparts]));
            }
        }
    }
}
// {ta, tb} of the segments this rank owns (device order): positions of their T1 / T2 inside the block of their virtual owner (= inside the part's
// reduce-scattered sums); ta + (first edge of the part - first edge of the rank) is the segment's place in the rank's all-gather slice
__global__ __launch_bounds__(256) void k_xt(const int32_t* pos_edge2, const EdgeInfo* einfo, const int32_t* ind_i, const int32_t* ind_j, const int32_t* rowptr,
                                            const int32_t* adj, const int32_t* node_lo, const int32_t* e_lo, const int32_t* prefB, int nv, int64_t t_half,
                                            int seg_lo, int seg_hi, int2* xt, int n) {
    for (int q = seg_lo + blockIdx.x * 256 + threadIdx.x; q < seg_hi; q += gridDim.x * 256) {
        const int e = pos_edge2[q], i = ind_i[e], j = ind_j[e];
        const int vo = owner_of_node(node_lo, nv, i);
        const int r0 = rowptr[j], r1 = rowptr[j + 1];
        const int first = nbrs_below(adj, r0, r1, node_lo[vo]);
        xt[q] = int2{e - e_lo[vo], (int)(t_half + prefB[(int64_t)vo * n + j] + ((einfo[q].slot_b - r0) - first))};
    }
}

int setup_node(desc_pgd* h, const desc_problem* prob, const desc_structure* s, const double* shared_rij) {
    const int64_t n = h->n, m = h->m, mp = h->m_pos;
    auto t0 = std::chrono::steady_clock::now();
    auto t_lap = t0;
    const bool timing = env_int("DESC_DEBUG_TIMING", 0) != 0;
    auto lap = [&](const char* what) {
        if (!timing) return;
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[desc_amd] setup_node %-22s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_lap).count());
        t_lap = now;
    };
    int rc;
    NodePlan P;
    // A structure built on this device brings its CSR, edge tables and sampled k along in HBM: the
    // per-edge tables and the cycle layout are then made by kernels and the host only plans.
    const bool dev_cycles = s->dev == h->device && s->d_k != nullptr;
    double* d_rij = nullptr;
    // node_seg != NULL: the staged form (natural order: one workgroup per node, the node's rotation blocks in the LDS)
    auto launch_layout_dev = [&](const int32_t* cum, const int32_t* src_start, const int32_t* pos, const int32_t* rowptr_d, uint32_t* pk, double* S0, uint8_t* perm,
                                 uint32_t* counts, int64_t nseg, const int32_t* node_seg) -> int {
        const int g = node_seg ? (int)std::max<int64_t>(1, n) : (int)std::min<int64_t>(4096, (nseg + 3) / 4);
        const size_t lds = node_seg ? (size_t)h->max_deg * 10 * sizeof(double) : 0;
        auto go = [&](auto kern) -> int {
            if (lds > 64 * 1024) DESC_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3(g), dim3(node_seg ? 512 : 256), lds, h->stream, cum, src_start, pos, s->d_ii, s->d_jj, s->d_k, s->d_tau, s->d_ktau, (uint64_t)s->seed, rowptr_d,
                               s->d_bits, s->d_rank, (int)s->words, s->d_adj_eid, d_rij, pk, S0, perm, counts, (int)nseg, node_seg, (int)n);
            return DESC_OK;
        };
        if (node_seg) return h->max_cnt <= 64 ? go(k_layout_node_dev<1, true>) : h->max_cnt <= 128 ? go(k_layout_node_dev<2, true>) : go(k_layout_node_dev<4, true>);
        return h->max_cnt <= 64 ? go(k_layout_node_dev<1, false>) : h->max_cnt <= 128 ? go(k_layout_node_dev<2, false>) : go(k_layout_node_dev<4, false>);
    };
    // One rank: packed words, S0_long (DESC_PGD.m:129-147) and the class order of every segment are computed NOW, in the structure's natural
    // order, under the host-side planning below; k_permute_segments moves them into the band-major order once that exists.  (Round 3 ran this
    // kernel -- 8.7 ms at C4 -- after the plan: the device idled through the planning, then the host through the kernel.)
    uint32_t *d_pk_nat = nullptr, *d_counts_nat = nullptr; double* d_S0_nat = nullptr; uint8_t* d_perm_nat = nullptr;
    const bool early = dev_cycles && h->world == 1 && mp > 0 && env_int("DESC_DEBUG_EARLY_LAYOUT", 1) != 0;
    if (early) {
        if (shared_rij) d_rij = const_cast<double*>(shared_rij);
        else {
            if ((rc = dalloc(h, &d_rij, 9 * (size_t)m))) return rc;
            if (m) DESC_HIP(hipMemcpy(d_rij, prob->rij, sizeof(double) * 9 * (size_t)m, hipMemcpyHostToDevice));
        }
        if ((rc = dalloc(h, &d_pk_nat, h->m_cycle + 8)) || (rc = dalloc(h, &d_S0_nat, h->m_cycle + 8)) || (rc = dalloc(h, &d_perm_nat, h->m_cycle + 8)) ||
            (rc = dalloc(h, &d_counts_nat, mp))) return rc;
        // the rotation blocks of a node's row in the LDS (80 B per slot) when the longest row fits: R_ki is then an LDS read (k_layout_node_dev<., STAGED>)
        int32_t* d_node_seg = nullptr;
        const bool staged = (size_t)h->max_deg * 80 <= 150 * 1024 && env_int("DESC_DEBUG_STAGED_LAYOUT", 1) != 0;
        if (staged) {
            if ((rc = dalloc(h, &d_node_seg, (size_t)n + 1))) return rc;
            hipLaunchKernelGGL(k_node_seg_start, dim3((unsigned)std::min<int64_t>(4096, (mp + 255) / 256)), dim3(256), 0, h->stream, s->d_pos, s->d_ii, mp, (int)n, d_node_seg);
        }
        if (s->ev_fill) DESC_HIP(hipStreamWaitEvent(h->stream, (hipEvent_t)s->ev_fill, 0));
        if ((rc = launch_layout_dev(s->d_cum, s->d_cum, s->d_pos, s->d_rowptr, d_pk_nat, d_S0_nat, d_perm_nat, d_counts_nat, mp, d_node_seg))) return rc;
        DESC_HIP(hipGetLastError());
    }
    // band sweep (i-rows of S in the LDS): segments of up to 64 cycles, every CSR row fits the LDS; DESC_DEBUG_VARIANT=2 keeps
    // the L2-sized bands of k_sweep_node for comparison
    int ncu = 256;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
    }
    // (tiny problems stay on k_sweep_node: with < 2 M cycles a 1024-thread workgroup per CU is mostly pipeline fill -- C1: 31 vs 20 us)
    const int force_band = env_int("DESC_DEBUG_VARIANT", 0);
    h->band_ok = force_band != VARIANT_NODE && h->max_cnt <= MAX_SEG_CYCLES && h->max_deg <= BAND_ROW_CAP && (h->m_cycle >= (2 << 20) || force_band == 3) &&
                 (int64_t)2 * m * 8 < (1ll << 32);          // 32-bit byte offsets into the CSR-aligned arrays (buffer instructions): m < 2.7e8 edges
    // exchange parts: the reduce-scatter of part c + 1 travels while part c is swept (band sweep only; DESC_SHARD_PARTS overrides, 1 = one reduce-scatter)
    // (segments of up to 64 cycles: every step plugin then runs on the band sweep; longer ones fall back to k_sweep_node for Adam, which sweeps in one launch)
    // every part's sweep writes band_grid (= ncu) partial pairs into its SHARD_PARTS / xparts of them: at most 4 parts with 256 CUs
    const int xparts = (h->world > 1 && h->band_ok && h->max_cnt <= 64) ? std::max(1, std::min({8, SHARD_PARTS / ncu, env_int("DESC_SHARD_PARTS", 2)})) : 1;
    if ((rc = make_node_plan(prob, s, h->max_deg, h->world, h->max_cnt <= 32 ? 32 : h->max_cnt <= 128 ? 16 : 8, h->band_ok ? band_row_cap(h->max_deg) : 0, P, xparts))) return rc;   // 8 waves x 64/lps segments
    h->xparts = P.xparts;
    h->band = P.band;
    lap("plan");
    const hvec<int32_t>& cum2 = P.cum2;
    const int64_t nch_all = (int64_t)P.chunk_seg.size() - 1;
    const int64_t ch_a = P.rank_chunk[h->rank], ch_b = P.rank_chunk[h->rank + 1];
    h->ch_lo = (int)ch_a; h->nchunks = (int)(ch_b - ch_a);
    h->seg_lo = P.chunk_seg[ch_a]; h->seg_hi = P.chunk_seg[ch_b];
    h->cyc_lo = cum2[h->seg_lo]; h->cyc_hi = cum2[h->seg_hi];
    h->rank_seg.assign((size_t)h->world + 1, 0);
    int64_t max_local = 0;
    for (int r = 0; r <= h->world; ++r) h->rank_seg[r] = P.chunk_seg[P.rank_chunk[r]];
    // exchange layout (k_xpos): a (virtual) owner has the edges whose smaller endpoint lies in its node range -- a contiguous range of the sorted edge list
    const int nv = h->world * h->xparts;
    hvec<int32_t> e_lo((size_t)nv + 1, (int32_t)m);
    for (int vo = 0; vo <= nv; ++vo)
        e_lo[vo] = (int32_t)(std::lower_bound(prob->ind_i, prob->ind_i + m, P.vnode[vo]) - prob->ind_i);
    int64_t max_local_v = 0;
    for (int r = 0; r < h->world; ++r) max_local = std::max<int64_t>(max_local, e_lo[(size_t)(r + 1) * h->xparts] - e_lo[(size_t)r * h->xparts]);
    for (int vo = 0; vo < nv; ++vo) max_local_v = std::max<int64_t>(max_local_v, e_lo[vo + 1] - e_lo[vo]);
    h->slice_len = max_local + 2 * SHARD_PARTS;     // S of the owned edges (edge order), then the workgroup partials (see k_unpack_S)
    h->slice_S = max_local;
    h->t_part = 2 * std::max<int64_t>(max_local_v, 1);
    if ((int64_t)nv * h->t_part >= (1ll << 31) - 1 || (int64_t)h->world * h->slice_len >= (1ll << 31) - 1)
        return fail(DESC_ERR_TOO_LARGE, "exchange buffers of %d ranks x %lld edges exceed the 32-bit positions of the exchange layout", h->world, (long long)max_local);
    h->xseg.assign((size_t)h->xparts + 1, 0); h->xslice_off.assign((size_t)h->xparts, 0);
    for (int c = 0; c <= h->xparts; ++c) h->xseg[c] = c < h->xparts ? std::min(std::max(P.vseg[(size_t)h->rank * h->xparts + c], h->seg_lo), h->seg_hi) : h->seg_hi;
    h->xseg[0] = h->seg_lo;
    for (int c = 0; c < h->xparts; ++c) h->xslice_off[c] = e_lo[(size_t)h->rank * h->xparts + c] - e_lo[(size_t)h->rank * h->xparts];
    const int64_t mcl = h->cyc_hi - h->cyc_lo;            // local cycles
    const int64_t nsl = h->seg_hi - h->seg_lo;            // local segments
    // band sweep: the work of every workgroup as a list of pieces (plan_band_pieces)
    hvec<PieceDesc> pieces; hvec<int32_t> piece_ptr;
    if (h->band_ok) {
        h->band_grid = ncu;
        bool jmajor = false;
        // one plan per exchange part (its segments only): a part is swept by a launch of its own
        h->xpiece_base.assign((size_t)h->xparts, 0); h->xpiece_ptr_base.assign((size_t)h->xparts, 0); h->xtail_first.assign((size_t)h->xparts, 0); h->xntail.assign((size_t)h->xparts, 0);
        h->band_rows = 0;
        for (int c = 0; c < h->xparts; ++c) {
            hvec<PieceDesc> pc; hvec<int32_t> pp; int rows_c = 0, tf = 0, nt = 0;
            const int64_t q0 = h->xseg[c], q1 = h->xseg[c + 1];
            const int max_tail = h->world > 1 ? std::max(0, std::min(MAX_TAIL_PIECES, SHARD_PARTS / h->xparts - h->band_grid)) : MAX_TAIL_PIECES;
            plan_band_pieces(prob, s, P, q0, q1, cum2[q0], (int64_t)cum2[q1] - cum2[q0], h->band_grid, pc, pp, rows_c, jmajor, &tf, &nt, max_tail);
            h->xpiece_base[c] = (int)pieces.size(); h->xpiece_ptr_base[c] = (int)piece_ptr.size(); h->xtail_first[c] = tf; h->xntail[c] = nt;
            pieces.insert(pieces.end(), pc.begin(), pc.end());
            piece_ptr.insert(piece_ptr.end(), pp.begin(), pp.end());
            h->band_rows = std::max(h->band_rows, rows_c);
        }
        h->band_tail_first = h->xtail_first[0]; h->band_ntail = h->xntail[0];
        for (int c = 1; c < h->xparts; ++c) h->band_ntail = std::max(h->band_ntail, h->xntail[c]);       // sweep_parts(): the largest part's count
        h->band_jmajor = jmajor;
        h->n_pieces = (int64_t)pieces.size(); h->n_bands = (int64_t)P.band_lo.size() - 1;
        for (const PieceDesc& pd : pieces) h->piece_row_entries += pd.row_len;
        if (timing) fprintf(stderr, "[desc_amd] band sweep: %zu bands, %zu pieces over %d workgroups, %s, rows <= %d\n", P.band_lo.size() - 1, pieces.size(),
                            h->band_grid, jmajor ? "j-block-major units" : "contiguous ranges", h->band_rows);
    }

    // CSR adjacency (neighbours ascending; single pass because Ind is sorted by (i,j))
    hvec<int32_t> rowptr, adj, adj_eid, eslot, eslot_b;
    if (!dev_cycles) {
        rowptr.assign((size_t)n + 1, 0); adj.resize((size_t)2 * m); adj_eid.resize((size_t)2 * m);
        for (int64_t e = 0; e < m; ++e) { rowptr[prob->ind_i[e] + 1]++; rowptr[prob->ind_j[e] + 1]++; }
        for (int64_t v = 0; v < n; ++v) rowptr[v + 1] += rowptr[v];
        // slot of every edge in its two endpoint rows (eslot: smaller endpoint, for S_vec extraction)
        eslot.resize((size_t)m); eslot_b.resize((size_t)m);
        hvec<int32_t> fill(rowptr.begin(), rowptr.end() - 1);
        for (int64_t e = 0; e < m; ++e) {
            const int32_t i = prob->ind_i[e], j = prob->ind_j[e];
            eslot[e] = fill[i]; eslot_b[e] = fill[j];
            adj[fill[i]] = j; adj_eid[fill[i]++] = (int32_t)e;
            adj[fill[j]] = i; adj_eid[fill[j]++] = (int32_t)e;
        }
    }
    lap("csr+eslot");
    // device-order tables of the segments: local cycle starts, start in the structure's natural cycle order, edge id; position of
    // every edge.  Device-built structures: k_seg_tables makes them from the plan's permutation (no host pass, two uploads instead of four)
    hvec<int32_t> cum_loc, src_start, pos_edge2, devpos;
    hvec<EdgeInfo> einfo;
    if (!dev_cycles) {
    cum_loc.resize((size_t)mp + 1); src_start.resize((size_t)mp); pos_edge2.resize((size_t)mp); devpos.assign((size_t)m, -1);
    cum_loc[mp] = cum2[mp] - (int32_t)h->cyc_lo;
    host_parallel(mp, [&](int64_t a, int64_t b) {
        for (int64_t q = a; q < b; ++q) {
            cum_loc[q] = cum2[q] - (int32_t)h->cyc_lo;                              // local cycle numbering (meaningful for owned segments)
            const int32_t l = P.order[q], e = s->pos_edge[l];
            src_start[q] = (int32_t)s->cum_ind[l];
            pos_edge2[q] = e; devpos[e] = (int32_t)q;
        }
    });
    }
    if (!dev_cycles) {
        einfo.resize((size_t)mp);
        host_parallel(mp, [&](int64_t a, int64_t b) {
            for (int64_t q = a; q < b; ++q) {
                const int32_t e = pos_edge2[q], i = prob->ind_i[e], j = prob->ind_j[e];
                einfo[q] = EdgeInfo{rowptr[i], rowptr[j], eslot[e], eslot_b[e]};
            }
        });
    }
    lap("einfo");
    hvec<uint32_t> kf; hvec<uint8_t> seg_perm; hvec<uint32_t> seg_counts; hvec<int2> adj_seg;
    if (!dev_cycles) {
        if ((rc = structure_ensure_host(const_cast<desc_structure*>(s)))) return rc;
    // k with the two mirror-present bits of the owned cycles, device order.  Inside a segment
    // the cycles are stored [(ik;j) only | both mirrors sampled | (jk;i) only | none] (ascending k
    // within a class): the column-sum pass then reads, for either endpoint, ONE run with the cycles that contribute
    // (a fraction ~n_sample/codeg of them), the per-segment arithmetic is order independent.
    kf.assign((size_t)mcl, 0u); seg_perm.assign((size_t)mcl, 0); seg_counts.assign((size_t)mp, 0u);   // counts: n_ionly | n_i << 9 | n_jonly << 18
    host_parallel(nsl, [&](int64_t a, int64_t b) {
        for (int64_t q = h->seg_lo + a; q < h->seg_lo + b; ++q) {
            const int64_t src = src_start[q], dst = cum_loc[q], cnt = cum2[q + 1] - cum2[q];
            int n_cls[4] = {0, 0, 0, 0};                      // class 0 i-only, 1 both, 2 j-only, 3 none
            auto cls = [&](int64_t t) { const bool fi = s->ikj[src + t] >= 0, fj = s->jki[src + t] >= 0; return fi ? (fj ? 1 : 0) : (fj ? 2 : 3); };
            for (int64_t t = 0; t < cnt; ++t) n_cls[cls(t)]++;
            int pos[4] = {0, n_cls[0], n_cls[0] + n_cls[1], n_cls[0] + n_cls[1] + n_cls[2]};
            for (int64_t t = 0; t < cnt; ++t) {
                const int o = pos[cls(t)]++;
                kf[dst + o] = (uint32_t)s->k[src + t] | (s->ikj[src + t] >= 0 ? 1u << 30 : 0u) | (s->jki[src + t] >= 0 ? 1u << 31 : 0u);
                seg_perm[dst + o] = (uint8_t)t;
            }
            seg_counts[q] = (uint32_t)n_cls[0] | (uint32_t)(n_cls[0] + n_cls[1]) << 9 | (uint32_t)n_cls[2] << 18;
        }
    });
    adj_seg.resize((size_t)2 * m);
    host_parallel(n, [&](int64_t a, int64_t b) {
        for (int64_t v = a; v < b; ++v)
            for (int32_t t = rowptr[v]; t < rowptr[v + 1]; ++t) {
                const int32_t q = devpos[adj_eid[t]];
                int2 rec{0, 0};
                if (q >= h->seg_lo && q < h->seg_hi) {       // only segments this rank owns
                    rec = slot_record(cum_loc[q], seg_counts[q], v < adj[t]);
                }
                adj_seg[t] = rec;
            }
    });
    }
    lap("host pack");
    // chunk tables: all chunks, local cycle numbering
    hvec<ChunkDesc> chunk_desc((size_t)std::max<int64_t>(nch_all, 1));
    for (int64_t t = 0; t < nch_all; ++t)
        chunk_desc[t] = ChunkDesc{cum2[P.chunk_seg[t]] - (int32_t)h->cyc_lo, cum2[P.chunk_seg[t + 1]] - (int32_t)h->cyc_lo, P.chunk_seg[t], P.chunk_seg[t + 1]};

    h->uc_default = (h->band_ok && (int64_t)2 * m * 8 > (12ll << 20)) ? 6 : 0;      // S beyond the L2s: S0 and the packed words in uncached memory (dalloc_stream)
    if ((rc = dalloc_stream(h, &h->d_S0, mcl + 8, 2))) return rc;   // +8: 16-byte tail reads
    if ((rc = dalloc_stream(h, &h->d_w[0], mcl + 8, 1))) return rc;
    if ((rc = dalloc_stream(h, &h->d_w[1], mcl + 8, 1))) return rc;
    if ((rc = dalloc_stream(h, &h->d_pk, mcl + 8, 4))) return rc;
    if ((rc = dalloc(h, &h->d_seg_perm, mcl))) return rc;
    if ((rc = dalloc(h, &h->d_einfo, mp))) return rc;
    if ((rc = dalloc(h, &h->d_rowptr, n + 1))) return rc;
    if ((rc = dalloc_stream(h, &h->d_adj_seg, 2 * m, 16))) return rc;
    if ((rc = dalloc(h, &h->d_src_start, mp))) return rc;
    if ((rc = dalloc(h, &h->d_eslot, m))) return rc;
    if ((rc = dalloc_stream(h, &h->d_S[0], 2 * m + 2, 32))) return rc;      // bits 32 / 64: experiments (profiles/r03_experiments.txt), never default; + 2: a 16-byte row load may end one double past 2m
    if ((rc = dalloc_stream(h, &h->d_S[1], 2 * m + 2, 32))) return rc;
    if ((rc = dalloc_stream(h, &h->d_T, 2 * m + 2, 64))) return rc;
    if ((rc = dalloc(h, &h->d_Svec, m))) return rc;
    if ((rc = dalloc(h, &h->d_chunk_desc, chunk_desc.size()))) return rc;
    if ((rc = dalloc(h, &h->d_rank_seg, (size_t)h->world + 1))) return rc;
    if ((rc = dalloc(h, &h->d_xpos, 2 * m))) return rc;
    if ((rc = dalloc(h, &h->d_spos, 2 * m))) return rc;
    if ((rc = dalloc(h, &h->d_xt, mp))) return rc;
    if (h->band_ok) {
        if ((rc = dalloc(h, &h->d_pieces, pieces.size()))) return rc;
        if ((rc = dalloc(h, &h->d_piece_ptr, piece_ptr.size()))) return rc;
        if (env_int("DESC_DEBUG_WGCLOCK", 0) && (rc = dalloc(h, &h->d_wg_clock, 3 * (size_t)h->band_grid))) return rc;
        if ((rc = dalloc(h, &h->d_ticket, 8))) return rc;                    // one ticket counter per exchange part
        DESC_HIP(hipMemsetAsync(h->d_ticket, 0, 8 * sizeof(int32_t), h->stream));
    }
    lap("alloc");
    int32_t *d_ii = nullptr, *d_jj = nullptr, *d_adj = nullptr, *d_adj_eid = nullptr, *d_pos_edge2 = nullptr;
    uint32_t* d_kf = nullptr;
    if (dev_cycles) {               // borrowed from the structure for the duration of this call
        d_ii = s->d_ii; d_jj = s->d_jj; d_adj = s->d_adj; d_adj_eid = s->d_adj_eid;
    } else {
        if ((rc = dalloc(h, &d_ii, m))) return rc;
        if ((rc = dalloc(h, &d_jj, m))) return rc;
        if ((rc = dalloc(h, &d_adj, 2 * m))) return rc;
        if ((rc = dalloc(h, &d_adj_eid, 2 * m))) return rc;
        if ((rc = dalloc(h, &d_kf, mcl))) return rc;
    }
    if ((rc = dalloc(h, &d_pos_edge2, mp))) return rc;
    const bool rij_up = d_rij != nullptr;                             // the early layout already has the rotations on the device
    if (rij_up) {}
    else if (shared_rij) d_rij = const_cast<double*>(shared_rij);     // the device problem's copy: no 72-B-per-edge upload
    else if ((rc = dalloc(h, &d_rij, 9 * (size_t)m))) return rc;
    hvec<int32_t> rank_seg32(h->rank_seg.begin(), h->rank_seg.end());
    int32_t *d_devpos = nullptr, *d_order_keep = nullptr;
    if (dev_cycles && s->ev_fill) {       // the structure's sampled cycles may still be on their way; a fault of that kernel is reported as its own
        const hipError_t ef = hipEventSynchronize((hipEvent_t)s->ev_fill);
        if (ef != hipSuccess) return fail(DESC_ERR_HIP, "cycle sampling kernel failed: %s", hipGetErrorString(ef));
    }
    if (dev_cycles) {
        int32_t* d_order = nullptr;
        if ((rc = dalloc(h, &d_devpos, m)) || (rc = dalloc(h, &d_order, mp))) return rc;
        if ((rc = upload(h, h->d_cum, cum2.data(), (size_t)mp + 1)) || (rc = upload(h, d_order, P.order.data(), (size_t)mp))) return rc;
        DESC_HIP(hipMemsetAsync(d_devpos, 0xFF, sizeof(int32_t) * std::max<int64_t>(1, m), h->stream));
        hipLaunchKernelGGL(k_seg_tables, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (mp + 256) / 256))), dim3(256), 0, h->stream,
                           d_order, s->d_pos, s->d_cum, h->d_cum, (int32_t)h->cyc_lo, h->d_src_start, d_pos_edge2, d_devpos, mp);
        DESC_HIP(hipStreamSynchronize(h->stream));       // d_order, the host sources of the copies
        if (early) d_order_keep = d_order; else dfree(h, d_order);
    } else {
    if ((rc = upload(h, h->d_cum, cum_loc.data(), (size_t)mp + 1))) return rc;
    if ((rc = upload(h, h->d_src_start, src_start.data(), (size_t)mp))) return rc;
    if ((rc = upload(h, d_pos_edge2, pos_edge2.data(), (size_t)mp))) return rc;
    }
    if ((rc = upload(h, h->d_chunk_desc, chunk_desc.data(), chunk_desc.size()))) return rc;
    if ((rc = upload(h, h->d_rank_seg, rank_seg32.data(), rank_seg32.size()))) return rc;
    // (a synchronous copy from pageable memory runs 2-3x faster than an asynchronous one on this runtime)
    if (!shared_rij && !rij_up && m) DESC_HIP(hipMemcpy(d_rij, prob->rij, sizeof(double) * 9 * (size_t)m, hipMemcpyHostToDevice));
    if (h->band_ok) {
        if ((rc = upload(h, h->d_pieces, pieces.data(), pieces.size()))) return rc;
        if ((rc = upload(h, h->d_piece_ptr, piece_ptr.data(), piece_ptr.size()))) return rc;
    }
    if (dev_cycles) {
        DESC_HIP(hipMemcpyAsync(h->d_rowptr, s->d_rowptr, sizeof(int32_t) * (n + 1), hipMemcpyDeviceToDevice, h->stream));
        hipLaunchKernelGGL(k_edge_slots, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (m + 255) / 256))), dim3(256), 0, h->stream,
                           d_ii, d_jj, s->d_rowptr, d_adj, d_pos_edge2, h->d_eslot, h->d_einfo, m, mp);
    } else {
        if ((rc = upload(h, h->d_einfo, einfo.data(), (size_t)mp))) return rc;
        if ((rc = upload(h, h->d_rowptr, rowptr.data(), (size_t)n + 1))) return rc;
        if ((rc = upload(h, h->d_adj_seg, adj_seg.data(), (size_t)2 * m))) return rc;
        if ((rc = upload(h, h->d_eslot, eslot.data(), (size_t)m))) return rc;
        if ((rc = upload(h, d_ii, prob->ind_i, (size_t)m))) return rc;
        if ((rc = upload(h, d_jj, prob->ind_j, (size_t)m))) return rc;
        if ((rc = upload(h, d_adj, adj.data(), (size_t)2 * m))) return rc;
        if ((rc = upload(h, d_adj_eid, adj_eid.data(), (size_t)2 * m))) return rc;
        if ((rc = upload(h, d_kf, kf.data(), (size_t)mcl))) return rc;
        if ((rc = upload(h, h->d_seg_perm, seg_perm.data(), (size_t)mcl))) return rc;
    }
    DESC_HIP(hipStreamSynchronize(h->stream));
    h->ms_upload = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    lap("upload");

    {   // persistent grid: exactly the workgroups that are co-resident (registers / LDS decide)
        int per_cu = 0;
        const auto* big = node_inst_of({32, 4});                          // the largest-register instance (constant step)
        if (!big) return DESC_ERR_STATE;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)big->kern[0], big->NT, 0) != hipSuccess || per_cu < 1) per_cu = 2;
        int64_t want = std::min<int64_t>(std::max(h->nchunks, 1), (int64_t)ncu * per_cu);
        h->grid = (int)(std::max<int64_t>(want, 8) + 7) / 8 * 8;
    }
    h->obj_grid = (int)std::min<int64_t>(SHARD_PARTS, std::max<int64_t>(1, (nsl + 3) / 4));     // sharded runs: its partials travel in the all-gather slice
    h->colsum_stride = (h->max_deg + 1) | 1;                 // odd stride: the 4 copies start on different banks
    // one node per workgroup: the dispatcher balances
    // ... in REVERSE node order (round 3).  The sweep before it ends with the last j-blocks, i.e. the weights of the segments with the largest
    // j are the freshest lines in the L2s, and the sweep after it begins with the first j-blocks, i.e. gathers T2 of the smallest j first: going
    // through the nodes from n-1 down to 0 the pass starts on what the sweep just wrote and ends on what the next sweep reads first.  C4
    // (profiles/r03_node_order.txt, alternating in one call): column sums 238 -> 232 us, the SWEEP 1193 -> 1129 us (-5.4 %); a hashed
    // shuffle: sweep -4 % but column sums +4 %; longest row first (the scheduling argument): erratic; C5, C2, C3: within noise.
    // DESC_DEBUG_NODE_ORDER: 0 ascending (round 2), 1 longest row first, 2 reverse (default), 3 hashed shuffle.
    // Sharded runs (round 4): only the nodes that have segments of this rank in their row are visited, and of their row only the run of CSR
    // slots those segments occupy (k_node_runs).  Measured per rank of 8 at C4 before that (profiles/r04_shard_w8_c4_before.json): 132 us
    // for an eighth of the cycles against 233 us for all of them on one GPU -- every rank started all n workgroups and walked whole rows.
    {
        hvec<int32_t> ord;
        hvec<int2> runs;
        ord.reserve((size_t)n);
        if (h->world > 1 && n > 0) {
            if ((rc = dalloc(h, &h->d_node_run, (size_t)n))) return rc;
            hipLaunchKernelGGL(k_node_runs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d_rowptr, d_adj, P.rank_node[h->rank], P.rank_node[h->rank + 1],
                               h->d_node_run, (int)n);
            runs.resize((size_t)n);
            DESC_HIP(hipStreamSynchronize(h->stream));
            DESC_HIP(hipMemcpy(runs.data(), h->d_node_run, sizeof(int2) * (size_t)n, hipMemcpyDeviceToHost));
            for (int64_t v = 0; v < n; ++v) if (runs[v].y > runs[v].x) ord.push_back((int32_t)v);
        } else
            for (int64_t v = 0; v < n; ++v) ord.push_back((int32_t)v);
        const int mode = env_int("DESC_DEBUG_NODE_ORDER", 2);
        if (mode == 2) std::reverse(ord.begin(), ord.end());
        else if (mode == 3) std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return mix64((uint64_t)x) < mix64((uint64_t)y); });
        else if (mode == 1) std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return P.rowptr[x + 1] - P.rowptr[x] > P.rowptr[y + 1] - P.rowptr[y]; });
        // sharded: rows with a short run of this rank's segments go to the back of the list -- k_colsum_node gives them a wave each
        h->colsum_long = (int)ord.size();
        if (!runs.empty() && 4 * COLSUM_SHORT <= ((h->max_deg + 1) | 1) && env_int("DESC_DEBUG_COLSUM_SHORT", 1)) {
            const auto mid = std::stable_partition(ord.begin(), ord.end(), [&](int32_t v) { return runs[v].y - runs[v].x > COLSUM_SHORT; });
            h->colsum_long = (int)(mid - ord.begin());
        }
        h->colsum_nodes = (int)ord.size();
        h->colsum_grid = h->colsum_long + (h->colsum_nodes - h->colsum_long + 3) / 4;     // workgroups (0: a rank without segments); the launch adds the bookkeeping workgroup
        if ((rc = dalloc(h, &h->d_node_order, ord.size())) || (rc = upload(h, h->d_node_order, ord.data(), ord.size()))) return rc;
        DESC_HIP(hipStreamSynchronize(h->stream));
    }
    if ((rc = prepare_colsum(h))) return rc;
    if (h->band_ok) {      // the band rows + the nv table in dynamic LDS: more than the 64 KiB default
        h->band_lds = ((size_t)h->band_rows + MAX_SEG_CYCLES + 1) * sizeof(double);
        for (int adam = 0; adam < (h->max_cnt <= 64 ? 2 : 1); ++adam) {      // every instance this handle can launch (band_adam_ok)
            const auto* k = band_inst_of(h, adam);
            if (!k) return DESC_ERR_STATE;
            for (auto kern : k->kern)
                if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->band_lds) != hipSuccess) { (void)hipGetLastError(); h->band_ok = false; }
        }
    }
    // the reference's demo sizes: the latency-lean sweep (DESC_DEBUG_VARIANT = 2 / 3 keep k_sweep_node / the band sweep for the cross-checks)
    h->small_ok = force_band == 0 && !h->band_ok && h->world == 1 && h->max_cnt <= 64 && h->m_cycle < (2 << 20) && env_int("DESC_DEBUG_SMALL", 1) != 0;
    const SweepShape small = small_shape(h->max_cnt);
    h->small_grid = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (nsl + 4 * (64 / small.lps) - 1) / (4 * (64 / small.lps))));
    h->kname = h->small_ok ? small_prefix(small) : h->band_ok ? band_prefix(band_shape(h, false)) : node_prefix(node_shape(h->max_cnt));

    lap("occupancy/attrs");
    hipEvent_t e0, e1;
    DESC_HIP(hipEventCreate(&e0)); DESC_HIP(hipEventCreate(&e1));
    (void)hipEventRecord(e0, h->stream);
    if (nsl > 0 && !dev_cycles) {
        int g = (int)std::min<int64_t>(4096, (nsl + 3) / 4);
        hipLaunchKernelGGL(k_layout_node, dim3(g), dim3(256), 0, h->stream, h->d_cum + h->seg_lo, d_pos_edge2 + h->seg_lo, d_ii, d_jj,
                           d_kf, h->d_rowptr, d_adj, d_adj_eid, d_rij, h->d_pk, h->d_S0, (int)nsl);
    } else if (dev_cycles) {
        // the structure's per-cycle arrays never left the device: lay them out in place
        uint32_t* d_counts = nullptr;
        if ((rc = dalloc(h, &d_counts, mp))) return rc;
        DESC_HIP(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * std::max<int64_t>(1, mp), h->stream));
        if (early) {            // computed in natural order under the planning: move the segments to their device positions
            hipLaunchKernelGGL(k_permute_segments, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(8192, (mp + 3) / 4))), dim3(256), 0, h->stream,
                               d_order_keep, s->d_cum, h->d_cum, d_pk_nat, d_S0_nat, d_perm_nat, d_counts_nat, h->d_pk, h->d_S0, h->d_seg_perm, d_counts, mp);
        } else if (nsl > 0)
            if ((rc = launch_layout_dev(h->d_cum + h->seg_lo, h->d_src_start + h->seg_lo, d_pos_edge2 + h->seg_lo, h->d_rowptr, h->d_pk, h->d_S0, h->d_seg_perm, d_counts + h->seg_lo, nsl, nullptr))) return rc;
        hipLaunchKernelGGL(k_adj_seg, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(2048, (n * 16 + 255) / 256))), dim3(256), 0, h->stream,
                           h->d_rowptr, d_adj, d_adj_eid, d_devpos, h->d_cum, d_counts, (int)h->seg_lo, (int)h->seg_hi, h->d_adj_seg, (int)n);
        DESC_HIP(hipStreamSynchronize(h->stream));
        dfree(h, d_devpos); dfree(h, d_counts);
        dfree(h, d_order_keep); dfree(h, d_pk_nat); dfree(h, d_S0_nat); dfree(h, d_perm_nat); dfree(h, d_counts_nat);
    }
    {   // exchange layout of the sharded runs (both paths have the CSR index, the edge list and the segment tables on the device by now)
        int32_t *d_node_lo = nullptr, *d_elo = nullptr, *d_prefB = nullptr;
        if ((rc = dalloc(h, &d_node_lo, (size_t)nv + 1)) || (rc = dalloc(h, &d_elo, (size_t)nv + 1)) || (rc = dalloc(h, &d_prefB, (size_t)nv * std::max<int64_t>(n, 1)))) return rc;
        if ((rc = upload(h, d_node_lo, P.vnode.data(), (size_t)nv + 1)) || (rc = upload(h, d_elo, e_lo.data(), (size_t)nv + 1))) return rc;
        if (n > 0) {
            const unsigned g16 = (unsigned)std::max<int64_t>(1, std::min<int64_t>(2048, (n * 16 + 255) / 256));
            hipLaunchKernelGGL(k_prefB, dim3(nv), dim3(1024), 0, h->stream, h->d_rowptr, d_adj, d_node_lo, d_prefB, (int)n);
            hipLaunchKernelGGL(k_xpos, dim3(g16), dim3(256), 0, h->stream, h->d_rowptr, d_adj, d_adj_eid, d_node_lo, d_elo, d_prefB, nv, h->xparts, h->world, h->t_part, h->slice_len,
                               h->d_xpos, h->d_spos, (int)n);
            if (nsl > 0)
                hipLaunchKernelGGL(k_xt, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(2048, (nsl + 255) / 256))), dim3(256), 0, h->stream, d_pos_edge2, h->d_einfo,
                                   d_ii, d_jj, h->d_rowptr, d_adj, d_node_lo, d_elo, d_prefB, nv, h->t_part / 2, (int)h->seg_lo, (int)h->seg_hi, h->d_xt, (int)n);
        }
        DESC_HIP(hipStreamSynchronize(h->stream));            // e_lo / rank_node: host sources of the copies
        DESC_HIP(hipGetLastError());
        dfree(h, d_node_lo); dfree(h, d_elo); dfree(h, d_prefB);
    }
    {   // the column-index stream of the column-sum pass (needs adj_seg and pk: both complete on the stream by now)
        uint32_t *d_rowsum = nullptr, *d_rowbase = nullptr;
        if ((rc = dalloc(h, &d_rowsum, n)) || (rc = dalloc(h, &d_rowbase, n)) || (rc = dalloc_stream(h, &h->d_moff, 2 * m, 16))) return rc;
        const unsigned g16 = (unsigned)std::max<int64_t>(1, std::min<int64_t>(2048, (n * 16 + 255) / 256));
        hipLaunchKernelGGL(k_midx_rowsum, dim3(g16), dim3(256), 0, h->stream, h->d_rowptr, h->d_adj_seg, d_rowsum, (int)n);
        hvec<uint32_t> rs((size_t)n), rb((size_t)n);
        DESC_HIP(hipStreamSynchronize(h->stream));
        DESC_HIP(hipMemcpy(rs.data(), d_rowsum, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
        uint64_t tot = 0;
        for (int64_t v = 0; v < n; ++v) { rb[v] = (uint32_t)tot; tot += rs[v]; }
        if (tot >= (1ull << 32)) return fail(DESC_ERR_TOO_LARGE, "column-index stream exceeds 2^32 entries");
        h->colsum_entries = (int64_t)tot;
        if ((rc = dalloc_stream(h, &h->d_midx, (size_t)tot + 8, 8))) return rc;
        {   // average run length (contributing cycles per segment and endpoint) decides the lanes per segment of the column sums
            const double avg_run = nsl > 0 ? (double)tot / (2.0 * (double)nsl) : 0.0;
            const int forced_cl = env_int("DESC_DEBUG_COLSUM_CL", 0);
            h->colsum_cl = forced_cl == 8 || forced_cl == 16 ? forced_cl : (avg_run > 0.0 && avg_run <= 10.5 ? 8 : 16);
            if (timing) fprintf(stderr, "[desc_amd] column sums: %.2f contributing cycles per segment and endpoint on average -> %d lanes per segment\n", avg_run, h->colsum_cl);
        }
        if ((rc = upload(h, d_rowbase, rb.data(), (size_t)n))) return rc;
        hipLaunchKernelGGL(k_midx_fill, dim3(g16), dim3(256), 0, h->stream, h->d_rowptr, h->d_adj_seg, d_rowbase, h->d_moff, (int)n);
        hipLaunchKernelGGL(k_midx_entries, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(8192, (2 * m * 16 + 255) / 256))), dim3(256), 0, h->stream,
                           h->d_adj_seg, h->d_moff, h->d_pk, h->d_midx, (int64_t)2 * m);
        DESC_HIP(hipStreamSynchronize(h->stream));
        dfree(h, d_rowsum); dfree(h, d_rowbase);
    }
    (void)hipEventRecord(e1, h->stream);
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipGetLastError();
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
    h->ms_cycle_d = ms;
    lap("layout kernels");
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (!dev_cycles) { dfree(h, d_ii); dfree(h, d_jj); dfree(h, d_adj); dfree(h, d_adj_eid); dfree(h, d_kf); }
    dfree(h, d_pos_edge2); if (!shared_rij) dfree(h, d_rij);
    if (e != hipSuccess) return fail(DESC_ERR_HIP, "k_layout_node: %s", hipGetErrorString(e));
    return DESC_OK;
}

}  // namespace desc

using namespace desc;

extern "C" {

// Test hook, host only (no device call): the band-sweep work plan of `rank` of `world` for `grid` workgroups -- bands, ranks' segment
// ranges, pieces -- checked for its invariants (every owned segment in exactly one piece, a piece inside one band, band rows within
// the LDS budget).  stats[8] = {bands, pieces, largest band's row entries, max / min cycles per workgroup, j-block-major?, seg_lo, seg_hi}.
int desc_debug_band_plan(const desc_problem* prob, const desc_structure* s, int32_t world, int32_t rank, int32_t grid, int64_t* stats) {
    if (!prob || !s || !stats || world < 1 || rank < 0 || rank >= world || grid < 1) return fail(DESC_ERR_INVALID, "bad argument");
    if (s->m_pos == 0) return fail(DESC_ERR_INVALID, "no edge with cycles");
    int32_t max_deg = 0;
    {
        hvec<int32_t> deg((size_t)prob->n, 0);
        for (int64_t e = 0; e < prob->m; ++e) { deg[prob->ind_i[e]]++; deg[prob->ind_j[e]]++; }
        for (int32_t d : deg) max_deg = std::max(max_deg, d);
    }
    if (max_deg > BAND_ROW_CAP) return fail(DESC_ERR_TOO_LARGE, "a row exceeds the LDS budget");
    NodePlan P;
    int rc = make_node_plan(prob, s, max_deg, world, s->max_cnt <= 32 ? 32 : s->max_cnt <= 128 ? 16 : 8, band_row_cap(max_deg), P);
    if (rc) return rc;
    const int64_t seg_lo = P.chunk_seg[P.rank_chunk[rank]], seg_hi = P.chunk_seg[P.rank_chunk[rank + 1]];
    const int64_t cyc_lo = P.cum2[seg_lo], mcl = P.cum2[seg_hi] - cyc_lo;
    hvec<PieceDesc> pieces; hvec<int32_t> piece_ptr; int band_rows = 0; bool jmajor = false;
    plan_band_pieces(prob, s, P, seg_lo, seg_hi, cyc_lo, mcl, grid, pieces, piece_ptr, band_rows, jmajor);
    const int64_t nbands = (int64_t)P.band_lo.size() - 1;
    hvec<uint8_t> seen((size_t)(seg_hi - seg_lo), 0);
    int64_t wmax = 0, wmin = INT64_MAX;
    for (int b = 0; b < grid; ++b) {
        int64_t cyc = 0;
        for (int32_t pc = piece_ptr[b]; pc < piece_ptr[b + 1]; ++pc) {
            const PieceDesc& pd = pieces[pc];
            if (pd.seg_lo < seg_lo || pd.seg_hi > seg_hi || pd.seg_lo >= pd.seg_hi) return fail(DESC_ERR_STATE, "piece %d out of the rank's range", pc);
            int64_t bd = 0;
            while (bd + 1 < nbands && P.bstart[bd + 1] <= pd.seg_lo) ++bd;
            if (pd.seg_hi > P.bstart[bd + 1]) return fail(DESC_ERR_STATE, "piece %d straddles two bands", pc);
            if (pd.row_lo != P.rowptr[P.band_lo[bd]] || pd.row_len != P.rowptr[P.band_lo[bd + 1]] - pd.row_lo || pd.row_len > BAND_ROW_CAP)
                return fail(DESC_ERR_STATE, "piece %d carries the wrong band rows", pc);
            for (int64_t q = pd.seg_lo; q < pd.seg_hi; ++q) {
                const int32_t i = prob->ind_i[s->pos_edge[P.order[q]]];
                if (i < P.band_lo[bd] || i >= P.band_lo[bd + 1]) return fail(DESC_ERR_STATE, "segment %lld is not in the band of its piece", (long long)q);
                if (seen[q - seg_lo]++) return fail(DESC_ERR_STATE, "segment %lld is in two pieces", (long long)q);
            }
            cyc += P.cum2[pd.seg_hi] - P.cum2[pd.seg_lo];
        }
        wmax = std::max(wmax, cyc); wmin = std::min(wmin, cyc);
    }
    for (size_t q = 0; q < seen.size(); ++q) if (!seen[q]) return fail(DESC_ERR_STATE, "segment %lld is in no piece", (long long)(q + seg_lo));
    stats[0] = nbands; stats[1] = (int64_t)pieces.size(); stats[2] = band_rows; stats[3] = wmax; stats[4] = wmin; stats[5] = jmajor ? 1 : 0;
    stats[6] = seg_lo; stats[7] = seg_hi;
    return DESC_OK;
}

}  // extern "C"

// The cycle structure of a PGD batch, built on the device (desc_pgd_batch_create_where, DESC_BUILD_DEVICE).
//
// batch.hip's host path runs build_structure_host once per problem, concatenates the results and uploads seven index arrays: from
// B = 16 on that costs more than the PGD loop it feeds.  Here the host does O(m) work only -- validation and the CSR of
// every problem with LOCAL ids (batch_csr_host) -- and five launches on the handle's stream make, for the whole batch at once, the very
// arrays the host path uploads, element for element:
//
//   k_bs_codeg    one wave per edge: the common neighbours of its endpoints are counted with cb_common_neighbours (cemp_batch.h, the
//                 routine of the batched CEMP and LP samplers); codeg[e], and 1 added to bin codeg of the problem's histogram of
//                 n_b + 1 int32 bins (integer atomics: order-free).
//   k_bs_plan     one wave per problem: batch_plan_rule (batch_structure.h) on its histogram -> m_pos, max_codeg, n_sample, m_cycle,
//                 max_cnt.  The B records are the ONLY read-back of the build; from them the host makes its refusals, the offsets, the
//                 workgroup table and the allocations.
//   k_bs_compact  one workgroup per problem, in edge order: pos_edge (batch-global edge ids), cum (batch-global cycle positions, every
//                 problem writes the closing entry of its own range, so cum[MP] = MC) and the edge -> segment table.
//   k_bs_sample   one wave per segment: the common neighbours staged in ascending k; all of them when codeg < n_sample, otherwise the
//                 n_sample smallest (sample_key(seed_b, LOCAL edge id, LOCAL k), k) pairs -- k_fill_cycles' rule -- written in
//                 ascending k together with e_ki = adj_eid[row i, position] and e_jk = adj_eid[row j, position], both plus the
//                 problem's edge offset (cb_common_neighbours returns both row positions).
//   k_bs_mirror   k_mirror's rule on batch-global positions: binary search of j (of i) in the sampled list of edge {i,k} ({j,k}).
//
// Keys and ids are local: problem b's arrays, less its offsets, are what desc_structure_build gives for the problem alone, whatever
// stands around it in the batch.  The LDS a launch declares is sized from the largest codegree of the batch and addressed with the
// segment's own codegree: it enters no result.
//
// Control flow.  No grid-wide barrier, no spinning on memory, nothing between workgroups but the integer histogram atomics.  Every loop
// is bounded by a row length, a codegree, an edge count or 96 probes.  k_bs_compact is the only kernel with workgroup barriers; its
// loop bound is the problem's edge count, uniform over the workgroup.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "batch_kernels.h"
#include "batch_structure.h"

namespace desc {
namespace {

struct BsArgs {
    const CbProb* prob;
    const int32_t* eprob;       // batch-global edge id -> problem
    const int32_t* ii;          // local endpoints of every edge
    const int32_t* jj;
    const int32_t* rowptr;      // problem b's n_b + 1 row starts at node_off[b] + b, counted inside the problem
    const int32_t* adj;         // 2 m_b local neighbour ids at 2 edge_off[b]
    const int32_t* adj_eid;     // 2 m_b local edge ids
    const BatchPlan* plan;
    int32_t* codeg;             // M
    int32_t* hist;              // problem b's n_b + 1 bins at node_off[b] + b
    const int64_t* seg_off;     // count + 1 (known after the read-back)
    const int64_t* cycle_off;
    int32_t* pos;               // MP batch-global edge ids
    int32_t* cum;               // MP + 1 batch-global cycle positions
    int32_t* poe;               // M: batch-global edge id -> batch-global segment, -1 without a cycle
    int32_t* kk;                // MC local third vertices
    int32_t* e_jk;              // MC batch-global edge ids
    int32_t* e_ki;
    int32_t* ikj;               // MC batch-global cycle positions, -1 where the mirror cycle was not sampled
    int32_t* jki;
    int32_t M, MP, n_sample_min, lds_cap, exact_only;
};

// inclusive prefix sum of an int over the 64 lanes of a wave
__device__ __forceinline__ int bs_incl_scan(int v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// the CSR rows of the endpoints of batch-global edge g
struct BsEdge { int b, e, i, j, ri, di, rj, dj, eo; const int32_t* adj; const int32_t* eid; uint64_t seed; };
__device__ __forceinline__ BsEdge bs_edge(const BsArgs& a, int g) {
    BsEdge q;
    q.b = a.eprob[g];
    const CbProb pd = a.prob[q.b];
    q.eo = pd.edge_off; q.seed = pd.seed;
    q.e = g - pd.edge_off;                                   // the edge's index in its problem's (i, j)-sorted list
    q.i = a.ii[g]; q.j = a.jj[g];
    const int32_t* rp = a.rowptr + pd.node_off + q.b;
    q.adj = a.adj + 2 * (int64_t)pd.edge_off;
    q.eid = a.adj_eid + 2 * (int64_t)pd.edge_off;
    q.ri = rp[q.i]; q.di = rp[q.i + 1] - q.ri;
    q.rj = rp[q.j]; q.dj = rp[q.j + 1] - q.rj;
    return q;
}

__global__ __launch_bounds__(256) void k_bs_codeg(BsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t g64 = wid; g64 < a.M; g64 += nw) {
        const int g = __builtin_amdgcn_readfirstlane((int)g64);
        const BsEdge q = bs_edge(a, g);
        const int cd = cb_common_neighbours(q.adj, q.ri, q.di, q.rj, q.dj, lane, 0, nullptr);      // counted only: nothing is staged
        if (lane == 0) {
            a.codeg[g] = cd;
            atomicAdd(&a.hist[a.prob[q.b].node_off + q.b + cd], 1);                                 // cd <= n_b - 2
        }
    }
}

__global__ __launch_bounds__(64) void k_bs_plan(BsArgs a, BatchPlan* plan) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;                            // three passes over n_b + 1 bins: one lane's work
    const CbProb pd = a.prob[b];
    BatchPlan r;
    batch_plan_rule(a.hist + pd.node_off + b, pd.n, a.n_sample_min, &r);
    plan[b] = r;
}

__global__ __launch_bounds__(256) void k_bs_compact(BsArgs a) {
    __shared__ int sf[4], sc[4];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const CbProb pd = a.prob[b];
    const int ns = a.plan[b].n_sample;
    int lbase = (int)a.seg_off[b];
    long long cbase = a.cycle_off[b];
    for (int e0 = 0; e0 < pd.m; e0 += 256) {
        const int e = e0 + (int)threadIdx.x;
        const int cd = e < pd.m ? a.codeg[pd.edge_off + e] : 0;
        const int f = cd > 0 ? 1 : 0, c = cd > 0 ? min(cd, ns) : 0;                                 // DESC_PGD.m:36-37, :45
        const int inf = bs_incl_scan(f, lane), inc = bs_incl_scan(c, lane);
        if (lane == 63) { sf[wv] = inf; sc[wv] = inc; }
        __syncthreads();
        int l = lbase + inf - f;
        long long cy = cbase + inc - c;
        for (int w = 0; w < wv; ++w) { l += sf[w]; cy += sc[w]; }
        if (e < pd.m) {
            if (f) { a.pos[l] = pd.edge_off + e; a.cum[l] = (int32_t)cy; a.poe[pd.edge_off + e] = l; }
            else a.poe[pd.edge_off + e] = -1;
        }
        lbase += sf[0] + sf[1] + sf[2] + sf[3];
        cbase += (long long)sc[0] + sc[1] + sc[2] + sc[3];
        __syncthreads();                                     // sf / sc are rewritten by the next chunk
    }
    if (threadIdx.x == 0) a.cum[a.seg_off[b + 1]] = (int32_t)a.cycle_off[b + 1];     // the closing entry of this problem's range
}

__global__ __launch_bounds__(256) void k_bs_sample(BsArgs a) {
    extern __shared__ unsigned long long bs_smem[];          // keys[4][lds_cap], then the packed row positions [4][lds_cap] as uint32
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int cap = a.lds_cap;
    unsigned long long* keys = bs_smem + (size_t)wv * cap;
    uint32_t* st = (uint32_t*)(bs_smem + (size_t)4 * cap) + (size_t)wv * cap;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t l64 = wid; l64 < a.MP; l64 += nw) {
        const int l = __builtin_amdgcn_readfirstlane((int)l64);
        const int g = a.pos[l];
        const BsEdge q = bs_edge(a, g);
        const int n_sample = a.plan[q.b].n_sample;
        const int base = a.cum[l];
        const int cd = cb_common_neighbours(q.adj, q.ri, q.di, q.rj, q.dj, lane, cap, st);         // ascending k; cd <= cap (checked on the host)
        auto put = [&](int c, uint32_t p) {                  // one cycle: k, {k,i} and {j,k} from the two row positions (DESC_PGD.m:87-88)
            const int xi = (int)(p & 0xFFFFu), xj = (int)(p >> 16);
            a.kk[c] = q.adj[q.ri + xi];
            a.e_ki[c] = q.eo + q.eid[q.ri + xi];
            a.e_jk[c] = q.eo + q.eid[q.rj + xj];
        };
        if (cd < n_sample) {                                 // DESC_PGD.m:83 samples iff codeg >= n_sample
            for (int t = lane; t < cd; t += 64) put(base + t, st[t]);
        } else {
            for (int t = lane; t < cd; t += 64) keys[t] = d_sample_key(q.seed, (uint64_t)q.e, (uint64_t)q.adj[q.ri + (int)(st[t] & 0xFFFFu)]);
            __builtin_amdgcn_wave_barrier();
            // Keep the n_sample smallest keys: a separator g with exactly n_sample keys <= g, by bisection on the key VALUE with
            // interpolated probes (the keys are uniform 64-bit hashes), every third probe halving -- k_fill_cycles' search.  Any such
            // separator selects the same set; where duplicate keys straddle the cut there is none, and the exact ranking decides.
            unsigned long long lo = 0, hi = ~0ull, sep = ~0ull;
            int c_lo = 0, c_hi = cd;
            bool have_lo = false, found = (cd == n_sample) && !a.exact_only;
            if (!found) sep = (unsigned long long)(((double)n_sample + 0.5) / (double)cd * 18446744073709549568.0);
            for (int it = 0; !found && !a.exact_only && it < 96; ++it) {
                int c = 0;
                for (int t0 = 0; t0 < cd; t0 += 64) { const int t = t0 + lane; c += __popcll(__ballot(t < cd && keys[t] <= sep)); }
                if (c == n_sample) { found = true; break; }
                if (c < n_sample) { lo = sep; c_lo = c; have_lo = true; } else { hi = sep; c_hi = c; }
                const unsigned long long bot = have_lo ? lo : 0ull;
                const unsigned long long span = hi - bot;
                if (span <= 1ull) break;                     // no value left in between
                unsigned long long step = span / 2ull;
                if (it % 3 != 2) {
                    const double frac = ((double)(n_sample - c_lo) + 0.5) / (double)(c_hi - c_lo + 1);
                    step = (unsigned long long)((double)span * frac);
                    step = step < 1ull ? 1ull : (step > span - 1ull ? span - 1ull : step);
                }
                sep = bot + step;
            }
            int outbase = 0;
            for (int t0 = 0; t0 < cd; t0 += 64) {
                const int t = t0 + lane;
                bool sel = false;
                if (t < cd) {
                    const unsigned long long kt = keys[t];
                    if (found) sel = kt <= sep;
                    else {                                   // exact ranking of the (key, k) pairs: positions ascend with k
                        int rk = 0;
                        for (int u = 0; u < cd; ++u) { const unsigned long long ku = keys[u]; rk += (ku < kt) || (ku == kt && u < t); }
                        sel = rk < n_sample;
                    }
                }
                const unsigned long long mk = __ballot(sel);
                if (sel) put(base + outbase + __popcll(mk & ((1ull << lane) - 1ull)), st[t]);
                outbase += __popcll(mk);
            }
        }
        __builtin_amdgcn_wave_barrier();                     // the staging area is reused by the wave's next segment
    }
}

__global__ __launch_bounds__(256) void k_bs_mirror(BsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t l = wid; l < a.MP; l += nw) {
        const int g = a.pos[l], i = a.ii[g], j = a.jj[g];
        for (int c = a.cum[l] + lane; c < a.cum[l + 1]; c += 64) {
            const int IK = a.poe[a.e_ki[c]];                 // an edge of a sampled triangle has a cycle: never -1
            int lo = a.cum[IK], hi = a.cum[IK + 1];
            const int end1 = hi;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (a.kk[mid] < j) lo = mid + 1; else hi = mid; }
            a.ikj[c] = (lo < end1 && a.kk[lo] == j) ? lo : -1;
            const int JK = a.poe[a.e_jk[c]];
            lo = a.cum[JK]; hi = a.cum[JK + 1];
            const int end2 = hi;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (a.kk[mid] < i) lo = mid + 1; else hi = mid; }
            a.jki[c] = (lo < end2 && a.kk[lo] == i) ? lo : -1;
        }
    }
}

}  // namespace

int batch_structure_device(BatchDevice* dev, const desc_problem* probs, int32_t count, int32_t n_sample_min, uint64_t seed,
                           const uint64_t* seeds, int32_t device, BatchBuilt* out, const PbSet* set) {
    // ---- host, O(m): validation (as the host path words it) and the per-problem CSR with local ids
    BatchCsr own;
    const BatchCsr& csr = set ? static_cast<const BatchCsr&>(*set) : own;
    int rc;
    if (!set) {
        if ((rc = batch_csr_host(probs, count, nullptr, &own, true))) return rc;
        for (int32_t b = 0; b < count; ++b) {
            const int32_t* rp = csr.rowptr.data() + csr.node_off[(size_t)b] + b;
            for (int64_t v = 0; v < probs[b].n; ++v)
                if (rp[v + 1] - rp[v] > CEMP_BATCH_MAX_DEGREE) return BATCH_BUILD_FALLBACK;             // row positions are packed in 16 bits
        }
    } else {                                           // the same rule from the set's host endpoints: its CSR may be on the device only
        hvec<int32_t> deg;
        for (int32_t b = 0; b < count; ++b) {
            deg.assign((size_t)probs[b].n, 0);
            for (int64_t e = csr.edge_off[(size_t)b]; e < csr.edge_off[(size_t)b + 1]; ++e) { ++deg[(size_t)csr.ii[(size_t)e]]; ++deg[(size_t)csr.jj[(size_t)e]]; }
            for (int32_t d : deg) if (d > CEMP_BATCH_MAX_DEGREE) return BATCH_BUILD_FALLBACK;
        }
    }
    out->edge_off = csr.edge_off;
    out->cycle_off.assign((size_t)count + 1, 0); out->seg_off.assign((size_t)count + 1, 0);
    out->plan.assign((size_t)count, BatchPlan{});
    if (count == 0) return DESC_OK;

    if ((rc = dev->open(device, "DESC_PGD_batch"))) return rc;             // nothing above touched the device
    const size_t M = (size_t)csr.M, NB = (size_t)csr.N + (size_t)count;
    hvec<CbProb> pr((size_t)count);
    for (int32_t b = 0; b < count; ++b)
        pr[(size_t)b] = CbProb{(int32_t)probs[b].n, (int32_t)probs[b].m, (int32_t)csr.node_off[(size_t)b], (int32_t)csr.edge_off[(size_t)b],
                               seeds ? seeds[b] : seed};
    BsArgs a{};
    BatchPlan* d_plan = nullptr;
    const int32_t *d_ii = nullptr, *d_jj = nullptr;
    hvec<int32_t> eprob;
    if ((rc = dev->upload(&a.prob, pr.data(), pr.size()))) return rc;
    if (!set) {
        eprob.resize(M);
        for (int32_t b = 0; b < count; ++b) {
            const size_t eo = (size_t)csr.edge_off[(size_t)b], m = (size_t)probs[b].m;
            std::fill(eprob.begin() + eo, eprob.begin() + eo + m, b);
        }
        if ((rc = dev->upload(&a.eprob, eprob.data(), M)) ||
            (rc = dev->upload(&d_ii, csr.ii.data(), M)) || (rc = dev->upload(&d_jj, csr.jj.data(), M)) ||
            (rc = dev->upload(&a.rowptr, csr.rowptr.data(), NB)) || (rc = dev->upload(&a.adj, csr.adj.data(), 2 * M)) ||
            (rc = dev->upload(&a.adj_eid, csr.adj_eid.data(), 2 * M))) return rc;
    } else {
        int32_t* d_eprob = nullptr;
        if ((rc = dev->mem.alloc(&d_eprob, M))) return rc;
        hipLaunchKernelGGL(k_batch_eprob<CbProb>, dim3((unsigned)count), dim3(256), 0, dev->stream, a.prob, d_eprob);
        DESC_HIP(hipGetLastError());
        a.eprob = d_eprob; d_ii = set->d_ii; d_jj = set->d_jj; a.rowptr = set->d_rowptr; a.adj = set->d_adj; a.adj_eid = set->d_adj_eid;
    }
    if ((rc = dev->mem.alloc(&a.codeg, M)) || (rc = dev->mem.alloc(&a.hist, NB)) || (rc = dev->mem.alloc(&d_plan, (size_t)count))) return rc;
    a.ii = d_ii; a.jj = d_jj; a.plan = d_plan;
    a.M = (int32_t)M; a.n_sample_min = n_sample_min;
    hipEvent_t ev[BATCH_BUILD_LAPS + 2] = {};      // start | codeg | plan || start | compact | sample | mirror
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int t = 0; t < BATCH_BUILD_LAPS + 2; ++t) if (e[t]) (void)hipEventDestroy(e[t]); } } guard{ev};
    for (int t = 0; t < BATCH_BUILD_LAPS + 2; ++t) DESC_HIP(hipEventCreate(&ev[t]));
    hipStream_t s = dev->stream;
    DESC_HIP(hipMemsetAsync(a.hist, 0, sizeof(int32_t) * std::max<size_t>(NB, 1), s));
    DESC_HIP(hipEventRecord(ev[0], s));
    if (M > 0) hipLaunchKernelGGL(k_bs_codeg, dim3((unsigned)grid_for((int64_t)M, 8192, 4)), dim3(256), 0, s, a);
    DESC_HIP(hipEventRecord(ev[1], s));
    hipLaunchKernelGGL(k_bs_plan, dim3((unsigned)count), dim3(64), 0, s, a, d_plan);
    DESC_HIP(hipEventRecord(ev[2], s));
    DESC_HIP(hipGetLastError());
    // ---- the only read-back of the build
    DESC_HIP(hipMemcpyAsync(out->plan.data(), d_plan, sizeof(BatchPlan) * (size_t)count, hipMemcpyDeviceToHost, s));
    DESC_HIP(hipStreamSynchronize(s));                 // the staging vectors above may go now, too
    int32_t max_codeg = 0;
    for (int32_t b = 0; b < count; ++b) max_codeg = std::max(max_codeg, out->plan[(size_t)b].max_codeg);
    if (max_codeg > BATCH_MAX_CODEG) return BATCH_BUILD_FALLBACK;          // the caller closes the device half and builds on the host
    // the refusals of the host path, in its order: a problem's own cycle count, n_sample, the totals of the batch
    for (int32_t b = 0; b < count; ++b)
        if (out->plan[(size_t)b].m_cycle >= (1ll << 31) - 1)
            return fail(DESC_ERR_TOO_LARGE, "problem %d: m_cycle = %lld exceeds 2^31-2", b, (long long)out->plan[(size_t)b].m_cycle);
    for (int32_t b = 0; b < count; ++b)
        if (out->plan[(size_t)b].n_sample > 64)
            return fail(DESC_ERR_INVALID, "problem %d: n_sample = %d exceeds 64 (segments longer than one wavefront): solve it with DESC_PGD", b,
                        out->plan[(size_t)b].n_sample);
    for (int32_t b = 0; b < count; ++b) {
        out->cycle_off[(size_t)b + 1] = out->cycle_off[(size_t)b] + out->plan[(size_t)b].m_cycle;
        out->seg_off[(size_t)b + 1] = out->seg_off[(size_t)b] + out->plan[(size_t)b].m_pos;
    }
    const int64_t MC = out->cycle_off[(size_t)count], MP = out->seg_off[(size_t)count];
    if (MC >= (1ll << 31) - 1)
        return fail(DESC_ERR_TOO_LARGE, "the batch holds %lld cycles in total: the 2^31-1 index budget is exceeded, split the batch", (long long)MC);
    // (a batch of 2^30 edges or more was refused by batch_csr_host)

    // ---- compaction, sampling, mirror maps
    if ((rc = dev->upload(&a.seg_off, out->seg_off.data(), out->seg_off.size())) ||
        (rc = dev->upload(&a.cycle_off, out->cycle_off.data(), out->cycle_off.size()))) return rc;
    if ((rc = dev->mem.alloc(&a.pos, (size_t)MP)) || (rc = dev->mem.alloc(&a.cum, (size_t)MP + 1)) || (rc = dev->mem.alloc(&a.poe, M)) ||
        (rc = dev->mem.alloc(&a.kk, (size_t)MC)) || (rc = dev->mem.alloc(&a.e_jk, (size_t)MC)) || (rc = dev->mem.alloc(&a.e_ki, (size_t)MC)) ||
        (rc = dev->mem.alloc(&a.ikj, (size_t)MC)) || (rc = dev->mem.alloc(&a.jki, (size_t)MC))) return rc;
    a.MP = (int32_t)MP;
    a.lds_cap = std::max(64, (max_codeg + 63) / 64 * 64);
    const char* ex = getenv("DESC_DEBUG_EXACT_SELECT");                   // tests: force the exact (tie-safe) ranking for every edge
    a.exact_only = (ex && atoi(ex) != 0) ? 1 : 0;
    const size_t lds = (size_t)4 * (size_t)a.lds_cap * (8 + 4);
    if (lds > 64 * 1024) return fail(DESC_ERR_STATE, "LDS budget exceeded (%zu bytes)", lds);
    DESC_HIP(hipEventRecord(ev[3], s));
    hipLaunchKernelGGL(k_bs_compact, dim3((unsigned)count), dim3(256), 0, s, a);
    DESC_HIP(hipEventRecord(ev[4], s));
    if (MP > 0) hipLaunchKernelGGL(k_bs_sample, dim3((unsigned)grid_for(MP, 8192, 4)), dim3(256), lds, s, a);
    DESC_HIP(hipEventRecord(ev[5], s));
    if (MP > 0) hipLaunchKernelGGL(k_bs_mirror, dim3((unsigned)grid_for(MP, 8192, 4)), dim3(256), 0, s, a);
    DESC_HIP(hipEventRecord(ev[6], s));
    DESC_HIP(hipGetLastError());
    DESC_HIP(hipStreamSynchronize(s));                 // seg_off / cycle_off were uploaded from the caller's vectors
    for (int t = 0; t < BATCH_BUILD_LAPS; ++t) {                        // laps 0-1 lie before the read-back, 2-4 behind it
        float ms = 0;
        const int e0 = t < 2 ? t : t + 1;
        DESC_HIP(hipEventElapsedTime(&ms, ev[e0], ev[e0 + 1]));
        out->ms_lap[t] = ms;
    }
    out->d_cum = a.cum; out->d_pos = a.pos; out->d_ejk = a.e_jk; out->d_eki = a.e_ki; out->d_ikj = a.ikj; out->d_jki = a.jki;
    out->d_kk = a.kk; out->d_ii = d_ii; out->d_jj = d_jj; out->d_codeg = a.codeg;
    return DESC_OK;
}

}  // namespace desc

extern "C" {

int32_t desc_pgd_batch_max_codeg(void) { return desc::BATCH_MAX_CODEG; }

int desc_test_batch_plan(const int32_t* hist, int32_t n, int32_t n_sample_min, int64_t* out) {
    if (!hist || !out || n < 0) return desc::fail(DESC_ERR_INVALID, "NULL argument or negative n");
    desc::BatchPlan r;
    desc::batch_plan_rule(hist, n, n_sample_min > 0 ? n_sample_min : 30, &r);
    out[0] = r.m_pos; out[1] = r.max_codeg; out[2] = r.n_sample; out[3] = r.m_cycle; out[4] = r.max_cnt;
    return DESC_OK;
}

}  // extern "C"
